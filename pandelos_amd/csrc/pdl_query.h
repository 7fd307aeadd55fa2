// pdl_query.h — K-query: one new genome scored against the dictionary that is already in HBM (pdl_query_scores,
// include/pandelos_amd.h), included from pdl_join.hip behind the join and K-order, whose finalize and ordering it reuses.
//
// Contract: the block computeScores(G) (library.cpp:409-527) returns for the UNION run — base genes 0..N-1, then the n query
// genes as genome G with ids N..N+n-1, same k.  The base context is only read.
//
//   Q-alpha  k_q_absent         query bytes against the base's letter-presence table (an absent letter changes the union's
//                               rank table, library.cpp:96-119): the smallest offending byte
//   Q-dict   pdl_query_dictionary (pdl_dict.hip)   K-rank with the base's RankParams, K-sort, K-rle: query records
//                               (rank, gene, count) in (rank, gene) order
//   Q-fold   k_q_fold           one thread: the base's last-record fold (k_fold_last_record) and the union's (Q1 below)
//   Q-match  k_q_match          per query record: its union group as base slice(s) + query slice(s), binary searches
//                               (both over one view, QView<KeyB, KeyQ, RK>: the base's key type, the query's, and whether the query
//                               is re-keyed — below; a plain query is <KeyT, KeyT, false>, chosen on the host by q_with_keys)
//   Q-rows   gene sort of the records (pdl_sort_pairs) + k_q_row_off: each query gene's records, in rank order
//   Q-join   k_q_join           one workgroup per query gene, LDS hash keyed by column; rows whose columns do not fit go to
//            k_q_join_hbm       the same row program on direct-addressed tables in HBM
//   Q-order  k_order_rows_wave / k_order_rows   the reference's emission order (chunk, first group, column)
//
// Option "query_rekey" (default off: the stages above, launched as ever).  On, Q-alpha is k_q_absent<LETTERS> — the absent bytes
// themselves, 256 bits, read by the host before Q-dict — and a query that brings one takes the same stages with RK set:
//   Q-dict   with the UNION's RankParams and key width (rk_query, pdl_rekey.h: base letters + all the query's)
//   Q-rebase k_q_up3, k_q_rebase (pdl_rekey.h)   the fold's three base ranks written up into the union's alphabet; every query
//                               record's key written back into the base's, with a flag where it holds a new letter
//   Q-fold, Q-match  <KeyB, KeyQ, true>: the same fold and description over union ranks; the view's up3() and bkey(i, none) hand
//                               them what Q-rebase left — only the searches in the base's keys take the record's rebased key
//                               (q_base_key), and none for a flagged record.  (KeyB, KeyQ) is (u32, u32), (u32, u64) or (u64, u64):
//                               a superset alphabet never needs fewer bits (pdl_with_keys_up, pdl_common.h)
// Q-rows, Q-join and Q-order read no key: they are the same launches.  The digit map between an alphabet and a superset of it
// is strictly increasing, so order and equality of k-mers are the same on both sides.
//
// Match.  The base postings are rank-group major: the rank of post[u] is keys_b[recpos[u]] (what pdl_get_dictionary reads).
// They are in rank order except for ONE record: when the base's last record (rank bmax) was alone in its rank,
// k_fold_last_record moved it into the group before it (rank r2), at its gene-order place.  Every rank of [gs, U) is r2
// except that record p, so a search for a rank below r2 runs over [0, gs), rank r2 is [gs, U) (minus p where the union
// does not fold it), rank bmax is {p}.  Binary search rather than a merge-path join: the query holds 1/(G+1) of the
// records, so log2(U) dependent probes per query record cost less than a pass over the whole dictionary.
//
// Q1 of the union (library.cpp:297-306).  The union's last record L (largest rank, then largest gene) joins the group of
// the largest rank below it when it is alone in its rank.  With qmax = largest query rank:
//   qmax > bmax, alone   L is the last query record qL; it joins the group of max(bmax, second query rank) — case (a);
//                        a base record p that the base had folded is an ordinary group of rank bmax again — case (b)
//   qmax >= bmax         otherwise no union fold; p (if folded) is again ordinary — cases (b), (d)
//   qmax <  bmax         L is the base's last record; if it was alone it joins max(r2, qmax): a query group when qmax > r2
//                        (p leaves [gs, U)) — case (c) — or r2 as in the base
// A group is described by {base slice, base record skipped, extra base record, query slice, extra query record}.
//
// Host side.  A single query is a run of ONE query and a chunk of a batch (pdl_query_batch.h) a run of several: both drivers are
// entry functions over the same stage functions — q_dictionary, q_match_out, q_gene_rows, q_join_and_order — which work on the
// run's QStageBufs (pdl_common.h: c->qb here, c->qbb there) and its QRun, index one control-word layout (Q_RUN_*, then Q_QRY_* per
// query) and leave one result view, pdl_query_cells.  pdl_run_query_device keeps what is a single query's own: the domain
// refusals, NewGenes, the single verdict of option "query_rekey", k_q_rowids, k_q_fold / k_q_match.
#pragma once
#include "pdl_sort.h"

constexpr uint32_t Q_NONE = 0xffffffffu;

struct QDesc {              // one query record's union group
    uint32_t blo, bhi;      // base postings [blo, bhi) ...
    uint32_t bskip;         // ... without this one (Q_NONE: none)
    uint32_t bextra;        // one more base posting (Q_NONE: none)
    uint32_t qlo, qhi;      // query records [qlo, qhi)
    uint32_t qextra;        // one more query record (Q_NONE: none)
    uint32_t key;           // order of the group among the row's groups (monotone in the group's rank)
};
__device__ __forceinline__ uint32_t q_size(const QDesc &d) {
    return (d.bhi - d.blo) - (d.bskip != Q_NONE ? 1u : 0u) + (d.bextra != Q_NONE ? 1u : 0u) + (d.qhi - d.qlo) + (d.qextra != Q_NONE ? 1u : 0u);
}

struct QFold {
    unsigned long long bmax, r2, tgt, extra_target;     // ranks in the alphabet the query is ranked in (the base's, or the union's: Q-rebase below)
    unsigned long long bmax_b;                          // bmax as the base's keys hold it
    uint32_t folded;        // the base folded its last record p into the group of rank r2 = [gs, U)
    uint32_t gs, p;
    uint32_t skip_p;        // in the union p is not part of [gs, U)
    uint32_t qL;            // query record the union folds into the group of rank tgt (Q_NONE: none)
    uint32_t has_extra;     // p joins the query group of rank extra_target
};

// Control words of a run — a single query (one query) or a chunk of a batch — in the run's `ctl` (u64): Q_RUN_WORDS for the run,
// then Q_QRY_WORDS per query; cleared at the start of every run, each word has one life.  q_query_ctl is the one accessor, for the
// kernels and for the host's copy (QCtlHost below).
enum : uint32_t {
    Q_RUN_RECORDS = 0,          // records of the run's dictionary (total of its dedup scan)
    Q_RUN_OVERFLOW_ROWS = 1,    // rows the LDS join handed to the HBM join
    Q_RUN_CELL_CURSOR = 2,      // staging cursor
    Q_RUN_EMITTED = 3,          // emitted cells (total of the row-count scan)
    Q_RUN_WIDE_ROWS = 4,        // order: rows of more than 256 cells
    Q_RUN_WORDS = 8,
};
enum : uint32_t {
    Q_QRY_RECORDS = 0,          // records of the query (a chunk's: its segment; the single query's are the run's)
    Q_QRY_BAD_BYTE = 1,         // 256 - smallest byte that is not in the base's alphabet (0: none)
    Q_QRY_COST = 2,             // genome cost
    Q_QRY_MATCHED = 3,          // matched records
    Q_QRY_BOUND = 4,            // staging bound
    Q_QRY_MAY_OVERFLOW = 5,     // rows that may overflow (more lookups than the LDS table holds keys)
    Q_QRY_EMITTED = 6,          // emitted cells (a chunk's; the single query's are the run's)
    Q_QRY_LETTERS = 8,          // option "query_rekey": 256 bits, the query's bytes that are not in the base's alphabet (4 words)
    Q_QRY_WORDS = 12,
};
template <class T> __host__ __device__ __forceinline__ T *q_query_ctl(T *ctl, uint32_t q) { return ctl + Q_RUN_WORDS + (size_t) q * Q_QRY_WORDS; }
constexpr size_t q_ctl_words(uint32_t nq) { return Q_RUN_WORDS + (size_t) nq * Q_QRY_WORDS; }

// Q-alpha: the bytes of `res` that the base's alphabet lacks — rare, so everything but the table test sits behind it.
//   LETTERS   false: the word at `words` is raised to 256 - byte, i.e. it ends as 256 - the smallest absent byte (0: none)
//             true:  the byte's bit is set in the 256 bits (32-bit words) at `words` (option "query_rekey")
//   BATCH     the words are those of the query the byte belongs to: `stride` words further per query, the query found by a
//             search of res_begin [nq + 1] (pdl_query_batch.h); false: one query, one atomic a thread
struct QAbsentArgs { const uint8_t *res; uint64_t n; uint32_t present[8]; const uint64_t *res_begin; uint32_t nq, stride; unsigned long long *words; };
template <bool LETTERS, bool BATCH>
__global__ __launch_bounds__(256) void k_q_absent(QAbsentArgs a) {
    uint32_t worst = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < a.n; i += (uint64_t) gridDim.x * 256) {
        const uint32_t b = a.res[i];
        if ((a.present[b >> 5] >> (b & 31)) & 1u) continue;
        unsigned long long *w = a.words;
        if constexpr (BATCH) {
            uint32_t lo = 0, hi = a.nq;                           // last query q with res_begin[q] <= i
            while (hi - lo > 1) { const uint32_t m = (lo + hi) >> 1; if (a.res_begin[m] <= i) lo = m; else hi = m; }
            w += (size_t) lo * a.stride;
        }
        if constexpr (LETTERS) atomicOr(reinterpret_cast<uint32_t *>(w) + (b >> 5), 1u << (b & 31));
        else if constexpr (BATCH) atomicMax(w, (unsigned long long) (256u - b));
        else worst = max(worst, 256u - b);
    }
    if constexpr (!LETTERS && !BATCH) if (worst) atomicMax(a.words, (unsigned long long) worst);
}
// the base's letters as the scan tests them: 256 bits
static void q_present_bits(const pdl_ctx *c, uint32_t present[8]) {
    for (int w = 0; w < 8; w++) present[w] = 0;
    for (int b = 0; b < 256; b++) if (c->alpha_present[b]) present[b >> 5] |= 1u << (b & 31);
}
// ... and its launch over n device bytes (none: nothing is queued)
template <bool LETTERS, bool BATCH>
static void q_scan_absent(pdl_ctx *c, const uint8_t *d_res, uint64_t n, const uint64_t *d_res_begin, uint32_t nq, uint32_t stride, unsigned long long *d_words) {
    if (!n) return;
    QAbsentArgs a{};
    a.res = d_res; a.n = n; a.res_begin = d_res_begin; a.nq = nq; a.stride = stride; a.words = d_words;
    q_present_bits(c, a.present);
    hipLaunchKernelGGL((k_q_absent<LETTERS, BATCH>), dim3((uint32_t) std::min<uint64_t>((n + 255) / 256, 1024)), dim3(256), 0, c->stream, a);
    PDL_HIP(hipGetLastError());
}
// The letter check shared with the append (pdl_dict.hip): the word the scan leaves at d_bad is turned into the refusal by
// pdl_fail_absent_byte (`who`: "query" / "appended").
void pdl_check_alphabet(pdl_ctx *c, const uint8_t *d_res, uint64_t n, unsigned long long *d_bad) {
    q_scan_absent<false, false>(c, d_res, n, nullptr, 1, 0, d_bad);
}
void pdl_fail_absent_byte(uint64_t bad_word, const char *who) {
    const uint32_t b = 256u - (uint32_t) bad_word;
    PDL_FAIL(PDL_ERR_UNSUPPORTED, "%s byte 0x%02x ('%c') is not in the base's alphabet: the union would rank k-mers differently", who, b,
             (b >= 32 && b < 127) ? (char) b : '?');
}

// first position in [lo, hi) whose rank is >= v (UPPER: > v); rank(position) ascends over the range
template <bool UPPER, class RankF>
__device__ __forceinline__ uint32_t q_bound(RankF rank, uint32_t lo, uint32_t hi, unsigned long long v) {
    while (lo < hi) { const uint32_t m = lo + ((hi - lo) >> 1); const unsigned long long r = rank(m); if (UPPER ? r <= v : r < v) lo = m + 1; else hi = m; }
    return lo;
}

// The base's postings as the searches see them.  The query records come with the accessors of a view (below) over its own index
// space: QView reads keys[recpos[j]], the batch's QBView (pdl_query_batch.h) its segment copy.
template <class KeyT> struct QBase {
    const KeyT *bkeys; const uint32_t *brecpos; const uint32_t *bvals; const uint2 *post; uint32_t U; uint64_t M;
    __device__ unsigned long long brank(uint32_t u) const { return (unsigned long long) bkeys[brecpos[u]]; }
    template <bool UPPER> __device__ uint32_t bbound(uint32_t lo, uint32_t hi, unsigned long long v) const {
        return q_bound<UPPER>([&](uint32_t u) { return brank(u); }, lo, hi, v);
    }
};
// Option "query_rekey", a query that brings letters the base lacks: it is ranked in the union's alphabet — keys of another type,
// KeyQ, where the union needs more bits — and searches the base's keys, which stay as they are.  What Q-rebase (pdl_rekey.h) left:
// per query record its key in the base's alphabet, or the flag that it has none (it holds a new letter: it equals no base rank);
// up3: the three ranks the fold reads from the base's keys, in the union's alphabet.  Every comparison of the fold and of
// q_describe is one between union ranks then; only the base searches take the record's key in the base's alphabet (q_base_key).
template <class KeyB> struct QRebased { const KeyB *bkey; const uint8_t *none; const unsigned long long *up3; };
// ... as a view holds it: `r` when the query is re-keyed (RK), nothing at all — an empty base — when it is not
template <class KeyB, bool RK> struct QRebasedIf { QRebased<KeyB> r; };
template <class KeyB> struct QRebasedIf<KeyB, false> {};
// What a view (QView here, QBView of pdl_query_batch.h) gives the fold and the description besides `b`, over its own index space
// of query records — here the records themselves, keys[recpos[i]]:
//   qrank(i)        record i's rank in the alphabet the query is ranked in
//   bkey(i, none)   its key in the base's alphabet (none: it has no such key); !RK: qrank(i), always one
//   up3()           QRebased::up3; !RK: null
template <class KeyB, class KeyQ, bool RK> struct QView : QRebasedIf<KeyB, RK> {
    QBase<KeyB> b;
    const KeyQ *qkeys; const uint32_t *qrecpos; const uint2 *qpost;
    __device__ unsigned long long qrank(uint32_t i) const { return (unsigned long long) qkeys[qrecpos[i]]; }
    __device__ unsigned long long bkey(uint32_t i, bool &none) const {
        if constexpr (RK) { none = this->r.none[i] != 0; return (unsigned long long) this->r.bkey[i]; }
        else { none = false; return qrank(i); }
    }
    __device__ const unsigned long long *up3() const { if constexpr (RK) return this->r.up3; else return nullptr; }
};

// The base half of the fold (see the head of this file): bmax, and when the base folded its last record: r2, gs, p.
// lonely: the base's last record is alone in its rank; has_r2: there is a group below it that it was folded into.
// up3 (null: the query is ranked in the base's alphabet): bmax and the ranks of the base's last two records in the union's.
template <class KeyT>
__device__ __forceinline__ QFold q_fold_base(const QBase<KeyT> &b, bool &lonely, bool &has_r2, const unsigned long long *up3 = nullptr) {
    QFold f{};
    f.p = Q_NONE; f.qL = Q_NONE;
    const uint32_t U = b.U;
    f.bmax = f.bmax_b = (unsigned long long) b.bkeys[b.M - 1];
    lonely = U == 1;                      // (U == 1: nothing to fold it into)
    has_r2 = false;
    if (U == 1) f.p = 0;
    else {
        const unsigned long long rl = b.brank(U - 1), rl2 = b.brank(U - 2);
        f.folded = (rl != f.bmax || rl2 != f.bmax) ? 1u : 0u;
        if (f.folded) {
            lonely = has_r2 = true;
            const bool r2_last = rl != f.bmax;
            f.r2 = r2_last ? rl : rl2;
            f.gs = b.template bbound<false>(0, U, f.r2);          // (p ranks above r2: the predicate rank < r2 stays monotone)
            if (up3) f.r2 = r2_last ? up3[1] : up3[2];            // (behind the last search that takes it as a base key)
            const uint32_t gl = b.bvals[b.M - 1];                 // gene of the folded record; [gs, U) ascends by gene, p included
            uint32_t lo = f.gs, hi = U;
            while (lo < hi) { const uint32_t m = lo + ((hi - lo) >> 1); if (b.post[m].x < gl) lo = m + 1; else hi = m; }
            if (b.brank(lo) != f.bmax) lo++;                      // the r2 record of the same gene sits in front of p
            f.p = lo;
        }
    }
    if (up3) f.bmax = up3[0];
    return f;
}

// The union half: Q1's cases (a)-(d) for the query whose records are the positions [s0, s1) (not empty) of the view's index
// space; f.qL is a position of that space.
template <class View>
__device__ __forceinline__ void q_fold_union(QFold &f, bool lonely, bool has_r2, const View &v, uint32_t s0, uint32_t s1) {
    const uint32_t Uq = s1 - s0;
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
}

// One thread: the folds of the base and of the union.  Launched only for a query with a k-mer (Mq >= 1), which therefore has a
// record: q_fold_union's [0, records) is not empty.
template <class KeyB, class KeyQ, bool RK>
__global__ void k_q_fold(QView<KeyB, KeyQ, RK> v, const unsigned long long *ctl, QFold *out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    bool lonely, has_r2;
    QFold f = q_fold_base(v.b, lonely, has_r2, v.up3());
    q_fold_union(f, lonely, has_r2, v, 0u, (uint32_t) ctl[Q_RUN_RECORDS]);
    *out = f;
}

// The union group of query record j, one of the records [s0, s1) of its query (positions of the view's index space).  The key is
// taken relative to s0: the same for a query on its own and as a segment of a batch.
// The rank record j's base searches look for, in the base's alphabet; none: there is no such rank (the record holds a letter the
// base lacks).  A record the union folds (j == f.qL) looks for f.tgt, which is the base's bmax — its key in the base's alphabet is
// kept beside it — or the rank of the query's last record but one, s1 - 2 (q_fold_union).
template <class View>
__device__ __forceinline__ unsigned long long q_base_key(const QFold &f, const View &v, uint32_t j, uint32_t s1, bool &none) {
    const unsigned long long bmax_b = f.bmax_b;       // (read up here, as a value: a choice between the ADDRESS of f's copy and of a key puts f in scratch)
    none = false;
    if (j != f.qL) return v.bkey(j, none);
    return f.tgt == f.bmax ? bmax_b : v.bkey(s1 - 2, none);
}

template <class View>
__device__ __forceinline__ QDesc q_describe(const QFold &f, const View &v, uint32_t j, uint32_t s0, uint32_t s1) {
    const auto &b = v.b;
    const auto qrank = [&](uint32_t i) { return v.qrank(i); };
    const unsigned long long eff = j == f.qL ? f.tgt : qrank(j);
    bool none;
    const unsigned long long beff = q_base_key(f, v, j, s1, none);
    QDesc d;
    d.blo = d.bhi = 0; d.bskip = d.bextra = d.qextra = Q_NONE;
    if (f.folded) {
        if (eff < f.r2) { if (!none) { d.blo = b.template bbound<false>(0, f.gs, beff); d.bhi = b.template bbound<true>(d.blo, f.gs, beff); } }
        else if (eff == f.r2) { d.blo = f.gs; d.bhi = b.U; if (f.skip_p) d.bskip = f.p; }
        else if (eff == f.bmax) { d.blo = f.p; d.bhi = f.p + 1; }
    } else if (!none) {
        d.blo = b.template bbound<false>(0, b.U, beff); d.bhi = b.template bbound<true>(d.blo, b.U, beff);
    }
    if (f.has_extra && eff == f.extra_target) d.bextra = f.p;
    const uint32_t qn = f.qL != Q_NONE ? s1 - 1 : s1;             // the searches among query records stay inside [s0, s1)
    d.qlo = q_bound<false>(qrank, s0, qn, eff); d.qhi = q_bound<true>(qrank, d.qlo, qn, eff);
    if (f.qL != Q_NONE && eff == f.tgt) d.qextra = f.qL;
    d.key = 2u * (d.qlo - s0) + (d.qhi > d.qlo ? 1u : 0u);
    return d;
}

// what the match (k_q_match, and k_qb_match of pdl_query_batch.h) leaves
struct QMatchOut {
    QDesc *desc; uint32_t *gene_key; uint32_t *row_lookups;
    unsigned long long *ctl;
};
// One thread per query record: its union group, the gene it sorts by, the row's lookups; cost and matched count of the query
template <class KeyB, class KeyQ, bool RK>
__global__ __launch_bounds__(256) void k_q_match(QView<KeyB, KeyQ, RK> v, const QFold *pf, QMatchOut o, uint64_t bound) {
    const QFold f = *pf;
    const uint32_t Uq = (uint32_t) o.ctl[Q_RUN_RECORDS];
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    unsigned long long cost = 0, matched = 0;
    if (j < Uq && j < bound) {
        const QDesc d = q_describe(f, v, j, 0u, Uq);
        const uint32_t sz = q_size(d);
        o.desc[j] = d;
        const uint32_t gene = v.qpost[j].x;
        o.gene_key[j] = gene;
        if (sz >= 2) { cost = sz; atomicAdd(&o.row_lookups[gene], sz); }
        matched = (j != f.qL && d.bhi > d.blo) ? 1ull : 0ull;
    }
#pragma unroll
    for (int s = PDL_WAVE / 2; s > 0; s >>= 1) { cost += __shfl_down(cost, s, PDL_WAVE); matched += __shfl_down(matched, s, PDL_WAVE); }
    if ((threadIdx.x & (PDL_WAVE - 1)) == 0) {
        if (cost) atomicAdd(q_query_ctl(o.ctl, 0) + Q_QRY_COST, cost);
        if (matched) atomicAdd(q_query_ctl(o.ctl, 0) + Q_QRY_MATCHED, matched);
    }
}

// row_off[g] = first position of gene g in the gene-sorted records; staging bound = sum of min(lookups, columns); rows whose
// lookups exceed `limit` (they may claim more columns than the LDS table of the join holds)
__global__ __launch_bounds__(256) void k_q_row_off(const uint32_t *gene_sorted, const unsigned long long *ctl, uint32_t n, uint32_t *row_off,
                                                   const uint32_t *row_lookups, uint32_t n_cols, uint32_t limit, unsigned long long *bound,
                                                   unsigned long long *wide) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    const uint32_t Uq = (uint32_t) ctl[Q_RUN_RECORDS];
    unsigned long long b = 0, w = 0;
    if (g <= n) {
        uint32_t lo = 0, hi = Uq;
        while (lo < hi) { const uint32_t m = lo + ((hi - lo) >> 1); if (gene_sorted[m] < g) lo = m + 1; else hi = m; }
        row_off[g] = lo;
        if (g < n) { b = min(row_lookups[g], n_cols); w = row_lookups[g] > limit ? 1ull : 0ull; }
    }
#pragma unroll
    for (int s = PDL_WAVE / 2; s > 0; s >>= 1) { b += __shfl_down(b, s, PDL_WAVE); w += __shfl_down(w, s, PDL_WAVE); }
    if ((threadIdx.x & (PDL_WAVE - 1)) == 0) {
        if (b) atomicAdd(bound, b);
        if (w) atomicAdd(wide, w);
    }
}

// ---- Q-join ------------------------------------------------------------------------------------------------------------
// The row program — q_row_lds, q_row_hbm — is also the batch's: k_qb_join / k_qb_join_hbm (pdl_query_batch.h) hand it the
// arguments of the row's own query.
constexpr int QJ_T = 256;
constexpr uint32_t QJ_HT_BITS = 12, QJ_HT = 1u << QJ_HT_BITS;
constexpr uint32_t QJ_LIMIT = QJ_HT - 2 * QJ_T;         // keys a row may claim before it goes to the HBM tables (< HT: probes end)
constexpr uint32_t QJ_SLOTS = QJ_HT / QJ_T;
constexpr int QH_WG = 16;                               // workgroups (each with its own tables) of the HBM kernel, at most

struct QJoinArgs {
    const uint2 *post, *qpost;
    const QDesc *desc;
    const uint32_t *rec_sorted;     // record indices, grouped by gene, rank order inside
    const uint32_t *row_off;        // [n + 1]
    const uint32_t *kseq_b, *kseq_q, *genome_b;
    uint32_t N, n, G1, k;           // G1 = G + 1 genomes of the union
    float *MS, *CM;                 // [n][G1], [N + n]
    uint32_t *row_base, *row_cnt;
    float *st_score, *st_perc, *st_tr;
    uint32_t *st_col, *st_first;
    unsigned long long *cell_cursor;
    uint32_t *overflow_rows;
    unsigned long long *n_overflow;
    uint8_t *hbm;                   // HBM kernel: per workgroup w, at w * 16 * (N + n) bytes: acc u64[N + n] | first u32[N + n] | touched u32[N + n]
};

// member m of a union group -> {column, count}
__device__ __forceinline__ uint2 q_member(const QJoinArgs &a, const QDesc &d, uint32_t m) {
    const uint32_t nb = (d.bhi - d.blo) - (d.bskip != Q_NONE ? 1u : 0u) + (d.bextra != Q_NONE ? 1u : 0u);
    if (m < nb) {
        uint32_t u;
        if (d.bextra != Q_NONE && m == nb - 1) u = d.bextra;
        else { u = d.blo + m; if (d.bskip != Q_NONE && u >= d.bskip) u++; }
        const uint2 b = a.post[u];
        return make_uint2(b.x, b.y & 0x7fffffffu);
    }
    m -= nb;
    const uint32_t j = m < d.qhi - d.qlo ? d.qlo + m : d.qextra;
    const uint2 q = a.qpost[j];
    return make_uint2(a.N + q.x, q.y & 0x7fffffffu);
}

// Walk the row's groups in chunks of QJ_T records: sizes scanned in LDS, then the chunk's lookups as one flat index space.
// add(col, packed sums, group key) returns false when the row must leave the table.
template <class AddF>
__device__ __forceinline__ void q_walk_row(const QJoinArgs &a, uint32_t g, QDesc *s_d, uint32_t *s_cnt, uint32_t *s_pre, uint32_t *s_stop, AddF add) {
    const uint32_t r0 = a.row_off[g], r1 = a.row_off[g + 1], row = a.N + g;
    const uint32_t lane = threadIdx.x & (PDL_WAVE - 1), wave = threadIdx.x / PDL_WAVE;
    for (uint32_t c0 = r0; c0 < r1; c0 += QJ_T) {
        uint32_t sz = 0;
        const uint32_t ri = c0 + threadIdx.x;
        if (ri < r1) {
            const uint32_t j = a.rec_sorted[ri];
            const QDesc d = a.desc[j];
            sz = q_size(d);
            if (sz < 2) sz = 0;
            s_d[threadIdx.x] = d;
            s_cnt[threadIdx.x] = a.qpost[j].y & 0x7fffffffu;
        }
        // exclusive scan of the sizes: inside the wave by shuffles, then the four wave totals
        uint32_t incl = sz;
#pragma unroll
        for (int s = 1; s < PDL_WAVE; s <<= 1) { const uint32_t t = __shfl_up(incl, s, PDL_WAVE); if ((int) lane >= s) incl += t; }
        if (lane == PDL_WAVE - 1) s_pre[QJ_T + 1 + wave] = incl;
        pdl_sync();
        uint32_t off = 0;
        for (uint32_t w = 0; w < wave; w++) off += s_pre[QJ_T + 1 + w];
        s_pre[threadIdx.x] = off + incl - sz;
        if (threadIdx.x == QJ_T - 1) s_pre[QJ_T] = off + incl;
        pdl_sync();
        const uint32_t total = s_pre[QJ_T];
        for (uint32_t t = threadIdx.x; t < total; t += QJ_T) {
            if (*(volatile uint32_t *) s_stop) break;
            uint32_t lo = 0, hi = QJ_T;                   // last record i with s_pre[i] <= t
            while (hi - lo > 1) { const uint32_t m = (lo + hi) >> 1; if (s_pre[m] <= t) lo = m; else hi = m; }
            const QDesc &d = s_d[lo];
            const uint2 mc = q_member(a, d, t - s_pre[lo]);
            if (mc.x == row) continue;                    // the self cell is zeroed (library.cpp:485-487): never emitted
            const uint32_t my = s_cnt[lo];
            const unsigned long long packed = (unsigned long long) min(mc.y, my) | ((unsigned long long) my << 21) | ((unsigned long long) mc.y << 42);
            if (!add(mc.x, packed, d.key)) { *s_stop = 1u; break; }
        }
        pdl_sync();
        if (*s_stop) return;
    }
}

// finalize one cell (library.cpp:493-517) and the two maxima (:405-407,513); returns the score (0: not emitted)
__device__ __forceinline__ float q_finalize(const QJoinArgs &a, uint32_t g, uint32_t col, unsigned long long acc, float &perc, float &tr) {
    const uint32_t my_k = a.kseq_q[g];
    const uint32_t other_k = col < a.N ? a.kseq_b[col] : a.kseq_q[col - a.N];
    const float threshold = 1.0f / (2.0f * (float) a.k);
    const float score = finalize_cell(acc, my_k, other_k, threshold, perc, tr);
    if (score > 0.0f) {
        const uint32_t genome = col < a.N ? a.genome_b[col] : a.G1 - 1;
        atomicMax(reinterpret_cast<uint32_t *>(a.MS) + (size_t) g * a.G1 + genome, __float_as_uint(score));    // non-negative: bit order = value order
        atomicMax(reinterpret_cast<uint32_t *>(a.CM) + col, __float_as_uint(score));
    }
    return score;
}

// One row on the LDS table: row g of `a` (uniform over the workgroup).  A row whose columns do not fit the table leaves
// overflow_id — what the HBM kernel of the caller finds the row by — in a.overflow_rows and emits nothing.
__device__ __forceinline__ void q_row_lds(const QJoinArgs &a, uint32_t g, uint32_t overflow_id) {
    __shared__ uint32_t s_key[QJ_HT], s_first[QJ_HT];
    __shared__ unsigned long long s_acc[QJ_HT];
    __shared__ QDesc s_d[QJ_T];
    __shared__ uint32_t s_cnt[QJ_T], s_pre[QJ_T + 1 + QJ_T / PDL_WAVE];
    __shared__ uint32_t s_nkeys, s_stop, s_ncell;
    __shared__ unsigned long long s_cbase;
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
            a.overflow_rows[i] = overflow_id;
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

__global__ __launch_bounds__(QJ_T) void k_q_join(QJoinArgs a) { q_row_lds(a, blockIdx.x, blockIdx.x); }

// One row on a workgroup's dense tables in HBM (acc, first, touched: all zero / all-ones first between rows — every touched
// entry is reset by the pass that emits it): the walk, the count pass, the emit pass.
__device__ __forceinline__ void q_row_hbm(const QJoinArgs &a, uint32_t g, unsigned long long *acc, uint32_t *first, uint32_t *touched) {
    __shared__ QDesc s_d[QJ_T];
    __shared__ uint32_t s_cnt[QJ_T], s_pre[QJ_T + 1 + QJ_T / PDL_WAVE];
    __shared__ uint32_t s_stop, s_ntouch, s_ncell, s_emit;
    __shared__ unsigned long long s_cbase;
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

// The rows k_q_join handed on, min(rows, QH_WG) workgroups with a table each.  Launched only when a row did overflow; the tables
// are allocated then, and cleared again whenever the column count they were laid out for is not this query's.
__global__ __launch_bounds__(QJ_T) void k_q_join_hbm(QJoinArgs a) {
    const uint32_t n_cols = a.N + a.n;
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(a.hbm + (size_t) blockIdx.x * n_cols * 16);
    uint32_t *first = reinterpret_cast<uint32_t *>(acc + n_cols);
    const uint32_t n_over = (uint32_t) *a.n_overflow;
    for (uint32_t w = blockIdx.x; w < n_over; w += gridDim.x) q_row_hbm(a, a.overflow_rows[w], acc, first, first + n_cols);
}

// the HBM tables of `slots` workgroups laid out for n_cols columns, in the state k_q_join_hbm leaves them: acc 0, first all ones
__global__ __launch_bounds__(256) void k_q_hbm_clear(uint8_t *hbm, uint32_t n_cols, uint32_t slots) {
    const uint64_t total = (uint64_t) n_cols * slots;
    for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t) gridDim.x * 256) {
        const uint64_t w = i / n_cols, col = i - w * n_cols;
        unsigned long long *acc = reinterpret_cast<unsigned long long *>(hbm + w * n_cols * 16);
        acc[col] = 0ull;
        reinterpret_cast<uint32_t *>(acc + n_cols)[col] = 0xffffffffu;
    }
}

__global__ __launch_bounds__(256) void k_q_rowids(uint32_t *ids, uint32_t base, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) ids[i] = base + i;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// The stages pdl_run_query_device and the batch's pdl_run_query_chunk_device (pdl_query_batch.h) share, over the run's QStageBufs
// (c->qb, c->qbb) and its description: q_dictionary, q_match_out, q_gene_rows, and everything behind the match, q_join_and_order.
struct QRun {
    uint32_t rows, queries;                         // genes of the run (the join's rows); queries
    const uint32_t *gene_begin, *d_gene_begin;      // [queries + 1] the queries' first rows: on the host, and (a chunk) on the device
    uint64_t residues, kmers;
    uint64_t max_cols;                              // columns of the widest union
    uint32_t hbm_cols;                              // columns the HBM tables are laid out for
    bool rekey;                                     // option "query_rekey": the run is ranked with the plan of c->qb.rk
    const char *who;                                // "query" / "query batch", and in a refusal query q is ...
    int64_t qa;                                     // ... "query <qa + q>:", the chunk's place in the caller's batch (-1: the single query, "query")
    bool single() const { return qa < 0; }
};

// the join's arguments as far as the base and the staging (five arrays of `cap` cells at `stf`) set them; the caller adds its own
// buffers, the query genes' count and the counters
static QJoinArgs q_join_args(pdl_ctx *c, float *stf, uint64_t cap) {
    QJoinArgs a{};
    a.post = c->post.as<uint2>(); a.kseq_b = c->kseq_len.as<uint32_t>(); a.genome_b = c->d_gen;
    a.N = c->N; a.G1 = c->G + 1; a.k = c->rp.k;
    a.st_score = stf; a.st_perc = stf + cap; a.st_tr = stf + 2 * cap;
    a.st_col = reinterpret_cast<uint32_t *>(stf + 3 * cap); a.st_first = reinterpret_cast<uint32_t *>(stf + 4 * cap);
    return a;
}

// One look of the host at n words on the device: the stretch of device work ends, the words come over (PinRead), and — unless
// this was the call's last look — the next stretch begins.
template <class T>
static void q_read_words(pdl_ctx *c, QSpans &spans, const void *d_src, size_t n, T *dst, bool more_work = true) {
    spans.end();
    {
        PinRead rd(c);
        const T *p = rd.add<T>(d_src, n);
        rd.sync();
        memcpy(dst, p, n * sizeof(T));
    }
    if (more_work) spans.begin();
}
// ... at all control words of a run of nq queries: the host's copy, indexed as the device's (q_query_ctl)
struct QCtlHost {
    std::vector<uint64_t> w;
    explicit QCtlHost(uint32_t nq) : w(q_ctl_words(nq)) {}
    void read(pdl_ctx *c, QSpans &spans, const void *d_ctl, bool more_work = true) { q_read_words(c, spans, d_ctl, w.size(), w.data(), more_work); }
    uint64_t run(uint32_t word) const { return w[word]; }
    uint64_t of(uint32_t q, uint32_t word) const { return q_query_ctl(w.data(), q)[word]; }
};

// The HBM tier, when some row has more lookups than the LDS table holds keys: the host looks whether a row left the table
// (*d_n_over); if so, tables (c->qb.hbm, shared by the single query and the batch) for W = min(rows, QH_WG) workgroups laid out for
// n_cols columns — clean tables of exactly that layout are taken as they are, any other are cleared, and the bookkeeping says what
// a later query will find (not clean from before the allocation until the clear is queued, so a throwing allocation leaves no
// stale claim) — then launch(tables, W).  The call's books (pdl_get_query_join_info) take the launch, its W and whether it cleared.
template <class LaunchF>
static void q_join_hbm_tier(pdl_ctx *c, QSpans &spans, const unsigned long long *d_n_over, uint32_t n_cols, LaunchF launch) {
    auto &q = c->qb;
    uint64_t n_over = 0;
    q_read_words(c, spans, d_n_over, 1, &n_over);
    if (!n_over) return;
    const uint32_t W = (uint32_t) std::min<uint64_t>(n_over, QH_WG);
    if (!q.hbm_clean || q.hbm_cols != n_cols || q.hbm_slots < W) {
        q.hbm_clean = false;
        q.hbm.alloc((size_t) W * n_cols * 16);
        hipLaunchKernelGGL(k_q_hbm_clear, dim3((uint32_t) std::min<uint64_t>(((uint64_t) W * n_cols + 255) / 256, 4096)), dim3(256), 0, c->stream,
                           q.hbm.as<uint8_t>(), n_cols, W);
        q.hbm_cols = n_cols; q.hbm_slots = W; q.hbm_clean = true;
        c->qj_call.hbm_clears++;
    }
    c->qj_call.hbm_launches++;
    c->qj_call.hbm_workgroups = std::max(c->qj_call.hbm_workgroups, W);
    launch(q.hbm.as<uint8_t>(), W);
    PDL_HIP(hipGetLastError());
}

// Q-order: the rows' final offsets (into fin_off; their total goes to *emitted) and the join's two ordering kernels, from the
// staging of `a` into `cells` (five arrays of `cap`); rowid: the rows' gene ids; max_cols: the widest union's columns
static void q_order_rows(pdl_ctx *c, const QJoinArgs &a, uint32_t *fin_off, uint32_t *rowid, float *cells, uint32_t n_rows, uint64_t cap,
                         uint64_t max_cols, unsigned long long *emitted, unsigned long long *wide_rows) {
    scan_and_apply(c, n_rows, RowCntFlag{a.row_cnt, nullptr}, FinOffApply{fin_off}, reinterpret_cast<uint64_t *>(emitted));
    OrderArgs o{};
    set_staged_cells(o, StagedCells{a.row_base, a.row_cnt, rowid, a.st_score, a.st_perc, a.st_tr, a.st_col, a.st_first}); o.fin_off = fin_off;
    o.c_score = cells; o.c_perc = cells + cap; o.c_tr = cells + 2 * cap;
    o.c_row = reinterpret_cast<int32_t *>(cells + 3 * cap); o.c_col = reinterpret_cast<int32_t *>(cells + 4 * cap);
    o.n_rows = n_rows; o.canonical = (c->flags & PDL_FLAG_CANONICAL_ORDER) ? 1u : 0u; o.pack_ok = max_cols < (1u << 22) ? 1u : 0u;
    o.wide_rows = reinterpret_cast<uint32_t *>(wide_rows);
    launch_order(c, o);
}

// The block as library.cpp:542-603 marshals it, for Z cells of n query genes: q_block_alloc sets the counts and allocates the
// ten arrays (a throw leaves what is allocated to pdl_free_scores); q_block_ids fills what the host knows once r.column is in.
static void q_block_alloc(pdl_ctx *c, pdl_scores &r, uint64_t Z, uint32_t n) {
    const uint32_t G1 = c->G + 1, NC = c->N + n;
    auto xm = [](size_t bytes) { void *p = malloc(bytes ? bytes : 1); if (!p) throw std::bad_alloc(); return p; };
    if (Z > 0xffffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "%llu cells exceed the block's 32-bit scoresCount", (unsigned long long) Z);
    r.scoresCount = (uint32_t) Z; r.rows = n; r.genomes = G1; r.sequences = NC;
    r.scores = (float *) xm(Z * 4); r.percs = (float *) xm(Z * 4); r.tr_percs = (float *) xm(Z * 4);
    r.row = (int32_t *) xm(Z * 4); r.column = (int32_t *) xm(Z * 4);
    r.first_seq_genome = (int32_t *) xm(Z * 4); r.second_seq_genome = (int32_t *) xm(Z * 4);
    r.max_genome_score = (float *) xm((size_t) n * G1 * 4); r.max_genome_score_col = (float *) xm((size_t) NC * 4);
    r.scoresMaxMappings = (int32_t *) xm((size_t) NC * 4);
}
static void q_block_ids(pdl_ctx *c, pdl_scores &r) {
    const uint32_t N = c->N, G = c->G;
    for (uint64_t i = 0; i < r.scoresCount; i++) {
        r.first_seq_genome[i] = (int32_t) G;
        const uint32_t col = (uint32_t) r.column[i];
        r.second_seq_genome[i] = col < N ? (int32_t) c->h_genome_of[col] : (int32_t) G;
    }
    for (uint32_t i = 0; i < N; i++) r.scoresMaxMappings[i] = 0x7fffffff;
    for (uint32_t g = 0; g < r.rows; g++) r.scoresMaxMappings[N + g] = (int32_t) g;
}

// Option "query_rekey": the verdict about the letters ONE query brings (256 bits, not empty) on its own — `who`: "query" /
// "query 3:" — and, with `adopt`, the plan for exactly these letters in c->qb.rk.  Both alphabets must give exact ranks.
static void q_rekey_verdict(pdl_ctx *c, const uint32_t letters[8], const char *who, bool adopt) {
    uint32_t b = 0;
    while (b < 255 && !((letters[b >> 5] >> (b & 31)) & 1u)) b++;
    const char shown = (b >= 32 && b < 127) ? (char) b : '?';
    const char *why = "";
    if (!pdl_query_rekey_base_exact(c, &why))
        PDL_FAIL(PDL_ERR_UNSUPPORTED, "%s byte 0x%02x ('%c') is not in the base's alphabet, and the base's ranks are %s: option query_rekey needs exact ranks "
                 "on the base's side and on the union's", who, b, shown, why);
    if (!pdl_query_rekey_plan(c, letters, adopt, &why))
        PDL_FAIL(PDL_ERR_UNSUPPORTED, "%s byte 0x%02x ('%c') is not in the base's alphabet, and the union's ranks would be %s: option query_rekey needs exact "
                 "ranks on the base's side and on the union's", who, b, shown, why);
    uint32_t brought = 0;
    for (int w = 0; w < 8; w++) brought += (uint32_t) __builtin_popcount(letters[w]);
    pdl_query_rekey_info &ri = c->qrk_call;
    ri.queries_rekeyed++;
    ri.letters_max = std::max(ri.letters_max, c->rp.base + brought);
}
// ... and what a pass that ran with the plan of c->qb.rk adds to the call's report (the stream is waited for when the pass is timed)
static void q_rekey_report(pdl_ctx *c, uint64_t records, bool rebased) {
    pdl_query_rekey_info &ri = c->qrk_call;
    ri.key_bits_max = std::max(ri.key_bits_max, c->qb.rk.rp.rank_bits);
    ri.records_rebased += records;
    if (rebased && c->opt_stage_timers) {
        PDL_HIP(hipStreamSynchronize(c->stream));
        ri.rebase_ms += c->qb.rk.span.total_ms();
    }
}
static bool q_any_letter(const uint32_t letters[8]) {
    uint32_t any = 0;
    for (int w = 0; w < 8; w++) any |= letters[w];
    return any != 0;
}

// The key types of a query's two sides and whether it is re-keyed, as types: f(KeyB{}, KeyQ{}, std::bool_constant<RK>{}) — the
// base's keys, the keys the query is ranked with (the plan of c->qb.rk when `rekey`, else the base's own) and RK = rekey.
template <class F>
static void q_with_keys(pdl_ctx *c, bool rekey, F &&f) {
    if (!rekey) pdl_with_key(c->key64, [&](auto key) { f(key, key, std::false_type{}); });
    else pdl_with_keys_up(c->key64, c->qb.rk.key64, [&](auto key_b, auto key_q) { f(key_b, key_q, std::true_type{}); });
}
template <class KeyB>
static QBase<KeyB> q_base(pdl_ctx *c) {
    return QBase<KeyB>{c->keys_b.as<KeyB>(), c->recpos.as<uint32_t>(), c->vals_b.as<uint32_t>(), c->post.as<uint2>(), (uint32_t) c->U, c->M};
}
// (RK: what pdl_query_rebase has left in c->qb.rk)
template <class KeyB>
static QRebased<KeyB> q_rebased(pdl_ctx *c) {
    auto &rk = c->qb.rk;
    return QRebased<KeyB>{rk.bkey.as<KeyB>(), rk.none.as<uint8_t>(), rk.up3.as<unsigned long long>()};
}
template <class KeyB, class KeyQ, bool RK>
static QView<KeyB, KeyQ, RK> q_view(pdl_ctx *c, const void *qkeys) {
    QView<KeyB, KeyQ, RK> v;
    v.b = q_base<KeyB>(c);
    v.qkeys = static_cast<const KeyQ *>(qkeys); v.qrecpos = c->qb.recpos.as<uint32_t>(); v.qpost = c->qb.post.as<uint2>();
    if constexpr (RK) v.r = q_rebased<KeyB>(c);
    return v;
}

// Q-dict over the genes a run has uploaded into w (res, off, koff), sized by the bound Mq; the record count stays on the device, at
// Q_RUN_RECORDS.  -> the buffer that holds the sorted keys, of q_key_bytes each.
static size_t q_key_bytes(const pdl_ctx *c, bool rekey) { return (rekey ? c->qb.rk.key64 : c->key64) ? 8 : 4; }
static const void *q_dictionary(pdl_ctx *c, pdl_ctx::QStageBufs &w, const QRun &r) {
    const uint64_t Mq = r.kmers;
    const size_t kb = q_key_bytes(c, r.rekey);
    w.keys_a.alloc(Mq * kb); w.keys_b.alloc(Mq * kb); w.vals_a.alloc(Mq * 4); w.vals_b.alloc(Mq * 4);
    w.recpos.alloc((Mq + 1) * 4); w.post.alloc(Mq * 8);
    return pdl_query_dictionary(c, r.rekey ? c->qb.rk.rp : c->rp, kb == 8, w.res.as<uint8_t>(), w.off.as<uint64_t>(), w.koff.as<uint64_t>(), r.rows, Mq, r.residues,
                                w.keys_a.p, w.keys_b.p, w.vals_a.as<uint32_t>(), w.vals_b.as<uint32_t>(), w.recpos.as<uint32_t>(), w.post.as<uint2>(),
                                reinterpret_cast<uint64_t *>(w.ctl.as<unsigned long long>() + Q_RUN_RECORDS));
}
// where the match writes: a description and a gene key per record, the rows' lookups (cleared) — and the rows' offsets behind them
static QMatchOut q_match_out(pdl_ctx *c, pdl_ctx::QStageBufs &w, const QRun &r) {
    w.desc.alloc(r.kmers * sizeof(QDesc)); w.gkey.alloc(r.kmers * 8); w.rec_sorted.alloc(r.kmers * 8);
    w.row_lookups.alloc(r.rows * 4ull); w.row_off.alloc((r.rows + 1) * 4ull);
    PDL_HIP(hipMemsetAsync(w.row_lookups.p, 0, r.rows * 4ull, c->stream));
    return QMatchOut{w.desc.as<QDesc>(), w.gkey.as<uint32_t>(), w.row_lookups.as<uint32_t>(), w.ctl.as<unsigned long long>()};
}
// Q-rows: each gene's records in rank order — a stable sort of the record indices by the gene key the match left (the records are in
// (rank, gene) order) — then row_off(gene keys, sorted) launches the run's row-offset kernel.  -> the sorted record indices
template <class RowOffF>
static const uint32_t *q_gene_rows(pdl_ctx *c, pdl_ctx::QStageBufs &w, const QRun &r, RowOffF row_off) {
    uint32_t *gk_in = w.gkey.as<uint32_t>(), *gk_out = gk_in + r.kmers;
    uint32_t *ix_in = w.rec_sorted.as<uint32_t>(), *ix_out = ix_in + r.kmers;
    pdl_sort_pairs<uint32_t, uint32_t>(c, gk_in, gk_out, ix_in, ix_out, r.kmers, std::max<uint32_t>(1, bit_length64(r.rows)), true,
                                       reinterpret_cast<const uint64_t *>(w.ctl.as<unsigned long long>() + Q_RUN_RECORDS), 0, true);
    row_off((const uint32_t *) gk_out);
    PDL_HIP(hipGetLastError());
    return ix_out;
}

// Everything behind the match: the host's look at the control words (a query's absent byte is refused here), the maxima cleared,
// Q-join — join(a) launches the LDS join over the run's rows, join_hbm(a, W) the HBM join of W workgroups —, Q-order, counts() for
// whatever the run counts per query behind it, and the closing look: one PinRead of the whole block.  qpost: the query records'
// postings as the row program indexes them; rec_sorted: q_gene_rows' (null: no k-mer); w.rowid, the rows' gene ids in their unions,
// is the caller's to fill before Q-order reads it — join(a) at the latest; it holds the run's rows from here on, and a caller that
// filled it earlier (a chunk's row offsets do) sized it so.  -> what the run leaves.
template <class JoinF, class JoinHbmF, class CountsF>
static pdl_query_cells q_join_and_order(pdl_ctx *c, pdl_ctx::QStageBufs &w, const QRun &r, const uint2 *qpost, const uint32_t *rec_sorted,
                                        JoinF join, JoinHbmF join_hbm, CountsF counts) {
    hipStream_t st = c->stream;
    QSpans &spans = w.spans;
    unsigned long long *ctl = w.ctl.as<unsigned long long>();
    const uint32_t N = c->N, G1 = c->G + 1, nq = r.queries, NT = r.rows;
    QCtlHost h(nq);
    h.read(c, spans, ctl);
    uint64_t bound = 0, may_overflow = 0;
    for (uint32_t q = 0; q < nq; q++) {
        if (h.of(q, Q_QRY_BAD_BYTE)) {
            char who[48] = "query";
            if (!r.single()) snprintf(who, sizeof(who), "query %u:", (uint32_t) r.qa + q);
            pdl_fail_absent_byte(h.of(q, Q_QRY_BAD_BYTE), who);
        }
        bound += h.of(q, Q_QRY_BOUND); may_overflow += h.of(q, Q_QRY_MAY_OVERFLOW);
    }
    const uint64_t Ut = h.run(Q_RUN_RECORDS);
    if (bound >= 0xffffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "%llu candidate cells exceed 32-bit cell positions", (unsigned long long) bound);

    const size_t ms_floats = (size_t) NT * G1, cm_floats = (size_t) nq * N + NT;
    w.MS.alloc(ms_floats * 4); w.CM.alloc(cm_floats * 4);
    PDL_HIP(hipMemsetAsync(w.MS.p, 0, ms_floats * 4, st));
    PDL_HIP(hipMemsetAsync(w.CM.p, 0, cm_floats * 4, st));
    const uint64_t cap = std::max<uint64_t>(bound, 1);
    uint64_t Z = 0;
    if (Ut) {
        w.row_base.alloc(NT * 4ull); w.row_cnt.alloc(NT * 4ull); w.fin_off.alloc((NT + 1) * 4ull); w.rowid.alloc(NT * 4ull); w.overflow.alloc(NT * 4ull);
        w.st.alloc(cap * 20); w.cells.alloc(cap * 20);
        QJoinArgs a = q_join_args(c, w.st.as<float>(), cap);
        a.qpost = qpost; a.desc = w.desc.as<QDesc>(); a.rec_sorted = rec_sorted; a.row_off = w.row_off.as<uint32_t>();
        a.kseq_q = w.kseq.as<uint32_t>(); a.n = NT; a.MS = w.MS.as<float>(); a.CM = w.CM.as<float>();      // (a.n: a chunk's rows take their own query's, qb_row_args)
        a.row_base = w.row_base.as<uint32_t>(); a.row_cnt = w.row_cnt.as<uint32_t>();
        a.cell_cursor = ctl + Q_RUN_CELL_CURSOR; a.overflow_rows = w.overflow.as<uint32_t>(); a.n_overflow = ctl + Q_RUN_OVERFLOW_ROWS;
        join(a);
        PDL_HIP(hipGetLastError());
        // (tables laid out for hbm_cols columns — the query's own count, a batch's widest union: those cleaned for another count are cleared again)
        if (may_overflow) q_join_hbm_tier(c, spans, a.n_overflow, r.hbm_cols, [&](uint8_t *hbm, uint32_t W) { a.hbm = hbm; join_hbm(a, W); });
        q_order_rows(c, a, w.fin_off.as<uint32_t>(), w.rowid.as<uint32_t>(), w.cells.as<float>(), NT, cap, r.max_cols, ctl + Q_RUN_EMITTED, ctl + Q_RUN_WIDE_ROWS);
        counts();
        PDL_HIP(hipGetLastError());
        h.read(c, spans, ctl, false);                             // the cursors and the per-query counts: one read
        const uint64_t staged = h.run(Q_RUN_CELL_CURSOR);
        Z = h.run(Q_RUN_EMITTED);
        if (Z > bound || staged > bound) PDL_FAIL(PDL_ERR_DEVICE, "%s join: %llu cells staged, bound %llu", r.who, (unsigned long long) staged, (unsigned long long) bound);
        c->qj_call.rows += NT; c->qj_call.may_overflow_rows += may_overflow; c->qj_call.overflow_rows += h.run(Q_RUN_OVERFLOW_ROWS);
    } else {
        spans.end();
    }
    if (r.rekey) q_rekey_report(c, Ut, r.kmers != 0);
    pdl_query_cells out;
    out.cells = w.cells.as<float>(); out.MS = w.MS.as<float>(); out.CM = w.CM.as<float>();
    out.Z = Z; out.cap = cap; out.nq = nq; out.genes = NT;
    out.gene_begin.assign(r.gene_begin, r.gene_begin + nq + 1); out.d_gene_begin = r.d_gene_begin;
    out.residues = r.residues; out.kmers = r.kmers; out.spans = &spans;
    out.cells_of.assign(nq, 0); out.records.resize(nq); out.matched.resize(nq); out.cost.resize(nq);
    for (uint32_t q = 0; q < nq; q++) {
        out.cells_of[q] = Ut ? h.of(q, Q_QRY_EMITTED) : 0;
        out.records[q] = h.of(q, Q_QRY_RECORDS); out.matched[q] = h.of(q, Q_QRY_MATCHED); out.cost[q] = h.of(q, Q_QRY_COST);
    }
    if (r.single()) { out.cells_of[0] = Z; out.records[0] = Ut; }       // (no segments, no per-query counts: the one query's are the run's)
    return out;
}

// The device half of a query: every stage up to the ordered cells, which stay where they are (pdl_run_query copies them out,
// K-place — pdl_place.h — filters them in HBM).
pdl_query_cells pdl_run_query_device(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, uint32_t n) {
    hipStream_t st = c->stream;
    auto &q = c->qb;
    const uint32_t N = c->N;
    const uint64_t NC64 = (uint64_t) N + n;
    if (NC64 >= 0x7fffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "%llu genes in the union exceed the 31-bit gene ids", (unsigned long long) NC64);
    const uint32_t NC = (uint32_t) NC64;
    const uint64_t Rq = offsets[n] - offsets[0];
    if (c->R + Rq >= 0xfffffff0ull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "more than 2^32 residues in the union need 64-bit stream positions");
    if (c->max_kseq >= (1ull << 20)) PDL_FAIL(PDL_ERR_UNSUPPORTED, "a base gene of %llu k-mers: queries need genes below 2^20 k-mers", (unsigned long long) c->max_kseq);
    const NewGenes genes(offsets, n, c->rp.k);
    for (uint32_t g = 0; g < n; g++)
        if (genes.kseq[g] >= (1u << 20)) PDL_FAIL(PDL_ERR_UNSUPPORTED, "query gene %u has %u k-mers: queries need genes below 2^20 k-mers", g, genes.kseq[g]);
    const uint64_t Mq = genes.M;
    if (Mq >= 0x7ffff000ull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "%llu query k-mers exceed the 31-bit record positions", (unsigned long long) Mq);
    QSpans &spans = q.spans;
    spans.start(st);
    spans.begin();

    // Q-alpha
    q.ctl.alloc(q_ctl_words(1) * sizeof(uint64_t));
    unsigned long long *ctl = q.ctl.as<unsigned long long>(), *qctl = q_query_ctl(ctl, 0);
    PDL_HIP(hipMemsetAsync(ctl, 0, q_ctl_words(1) * sizeof(uint64_t), st));
    genes.upload(c, residues);
    // option "query_rekey": the letters themselves come to the host before the dictionary is made; a query that brings one is
    // ranked with the union's table (base letters + ALL its letters, genes shorter than k included, as a build counts them)
    bool rekey = false;
    if (c->opt_query_rekey && Rq) {
        q_scan_absent<true, false>(c, q.res.as<uint8_t>(), Rq, nullptr, 1, 0, qctl + Q_QRY_LETTERS);
        uint32_t letters[8];
        q_read_words(c, spans, qctl + Q_QRY_LETTERS, 8, letters);
        if (q_any_letter(letters)) { q_rekey_verdict(c, letters, "query", true); rekey = true; }
    }
    if (!rekey) pdl_check_alphabet(c, q.res.as<uint8_t>(), Rq, qctl + Q_QRY_BAD_BYTE);
    const uint32_t gene_begin[2] = {0, n};
    // (tables laid out for THIS query's column count)
    const QRun run{n, 1, gene_begin, nullptr, Rq, Mq, NC, NC, rekey, "query", -1};

    // Q-dict, Q-fold, Q-match, Q-rows (sized by the bound Mq; the record count stays on the device until the look behind them)
    const uint32_t *rec_sorted = nullptr;
    if (Mq) {
        const void *qkeys = q_dictionary(c, q, run);
        q.fold.alloc(sizeof(QFold));
        const QMatchOut mo = q_match_out(c, q, run);
        const dim3 grid_m((uint32_t) ((Mq + 255) / 256));
        // (re-keyed: Q-rebase first, then fold and match in two alphabets — the base's key type for its keys, the union's for the query's)
        q_with_keys(c, rekey, [&](auto key_b, auto key_q, auto rk) {
            using KeyB = decltype(key_b);
            using KeyQ = decltype(key_q);
            constexpr bool RK = decltype(rk)::value;
            if constexpr (RK) pdl_query_rebase(c, qkeys, q.recpos.as<uint32_t>(), ctl + Q_RUN_RECORDS, Mq);
            const QView<KeyB, KeyQ, RK> v = q_view<KeyB, KeyQ, RK>(c, qkeys);
            hipLaunchKernelGGL((k_q_fold<KeyB, KeyQ, RK>), dim3(1), dim3(64), 0, st, v, (const unsigned long long *) ctl, q.fold.as<QFold>());
            hipLaunchKernelGGL((k_q_match<KeyB, KeyQ, RK>), grid_m, dim3(256), 0, st, v, (const QFold *) q.fold.as<QFold>(), mo, Mq);
        });
        PDL_HIP(hipGetLastError());
        rec_sorted = q_gene_rows(c, q, run, [&](const uint32_t *gene_sorted) {
            hipLaunchKernelGGL(k_q_row_off, dim3((n + 1 + 255) / 256), dim3(256), 0, st, gene_sorted, (const unsigned long long *) ctl, n, q.row_off.as<uint32_t>(),
                               (const uint32_t *) q.row_lookups.as<uint32_t>(), NC, QJ_LIMIT, qctl + Q_QRY_BOUND, qctl + Q_QRY_MAY_OVERFLOW);
        });
    }
    // the look, Q-join, Q-order: the rows are the query's genes N.., their arguments the same for all
    return q_join_and_order(c, q, run, q.post.as<uint2>(), rec_sorted,
        [&](const QJoinArgs &a) {
            hipLaunchKernelGGL(k_q_rowids, dim3((n + 255) / 256), dim3(256), 0, st, q.rowid.as<uint32_t>(), N, n);
            hipLaunchKernelGGL(k_q_join, dim3(n), dim3(QJ_T), 0, st, a);
        },
        [&](const QJoinArgs &a, uint32_t W) { hipLaunchKernelGGL(k_q_join_hbm, dim3(W), dim3(QJ_T), 0, st, a); },
        [] {});
}

void pdl_run_query(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, uint32_t n, pdl_scores *out, pdl_query_info *info) {
    hipStream_t st = c->stream;
    const uint32_t G1 = c->G + 1, NC = c->N + n;
    const pdl_query_cells run = pdl_run_query_device(c, residues, offsets, n);
    const uint64_t Z = run.Z;

    // Q-copy: straight into the block's arrays
    pdl_scores r{};
    try {
        q_block_alloc(c, r, Z, n);
        if (Z) {
            void *dst[5] = {r.scores, r.percs, r.tr_percs, r.row, r.column};
            for (int i = 0; i < 5; i++) PDL_HIP(hipMemcpyAsync(dst[i], run.cells + (size_t) i * run.cap, Z * 4, hipMemcpyDeviceToHost, st));
        }
        PDL_HIP(hipMemcpyAsync(r.max_genome_score, run.MS, (size_t) n * G1 * 4, hipMemcpyDeviceToHost, st));
        PDL_HIP(hipMemcpyAsync(r.max_genome_score_col, run.CM, (size_t) NC * 4, hipMemcpyDeviceToHost, st));
        PDL_HIP(hipStreamSynchronize(st));
    } catch (...) { pdl_free_scores(&r); throw; }
    q_block_ids(c, r);
    *out = r;
    if (info) run.info_of(0, run.residues, run.kmers, run.device_ms(), info);
}
