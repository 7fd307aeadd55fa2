// pdl_place_batch.h — K-place for a batch: q new genomes placed into the gene families that are already built, each on its own
// (pdl_place_batch, pdl_placement_batch_of_edges; included from pdl_bbh.hip behind pdl_place.h).
//
// Contract: placement j is what pdl_place_query returns for genome j alone — ids are query j's own union ids (its genes are
// N..N+n_j-1 of genome G).  The queries never see each other; the base context is only read.
//
// Per chunk of the query batch (pdl_query_batch.h cuts the chunks), on one stream, no cell crosses PCIe; the stages of pdl_place.h
// run ONCE over the chunk (place_run with the chunk's layout).  What a chunk adds to them:
//
//   B-alpha .. B-order   pdl_run_query_chunk_device: the chunk's ordered cells, MS and CM stay in HBM, query after query (pdl_query_cells)
//   P-bbh      with BbhQueryChunk over all cells of the chunk: a cell's row is an id of its own query's union, so the query comes
//              from the cell's index against the per-query cell offsets; MS row = gene_begin[q] + (row - N), the CM slice at
//              q * N + gene_begin[q], inter_max [q][G + 1], thr [chunk gene].  A query's phase-1 and phase-2 edges are one
//              stretch each, its counts the prefixes at its first cell (k_pick_prefixes); one PinRead.  All of it is
//              bbh_edges / bbh_read_counts / bbh_copy_out of pdl_bbh.hip with the queries as blocks, over K-place's own BbhBufs
//   PB-check   k_place_check_batch (callers' lists only): every list against its OWN [0, N + n_q) and for base-base edges, in one
//              launch, before any id indexes anything; the first failing query leaves by an atomicMax
//   flat ids   query q's own id x is shift[q] + x, shift[q] = q * N + gene_begin[q] — the queries' unions [N + n_q] one behind the
//              other, as the CM slices lie; a tree's root is its query's smallest own id.  PlaceChunk finds the query of an edge, a
//              chunk gene or a flat id by a search in the per-query offsets (last_le), uploaded once per run
//   the cut    groups come out in (query, label) order, so a query's groups, members and base components are one stretch of the
//              chunk's arrays each: place_run cuts them out and translates them to the query's own ids on the host
//
// The per-query copies of the base's labels and the label-indexed group table take 8 (N + n_q) bytes per query; a chunk is cut
// where its flat ids would reach 2^31 (a chunk of one always fits).
#pragma once

#include "pdl_place.h"

// last q in [0, n) with at[q] <= v (empty stretches lie before it)
template <class T>
static __device__ __forceinline__ uint32_t last_le(const T *at, uint32_t n, T v) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint32_t m = (lo + hi) >> 1; if (at[m] <= v) lo = m; else hi = m; }
    return lo;
}

// the queries of a chunk: `part` = the query of cell i
struct BbhQueryChunk {
    const uint32_t *genome_b, *gene_begin, *cell_begin; uint32_t N, G, nq;
    __device__ uint32_t part(uint32_t i) const { return last_le(cell_begin, nq, i); }
    __device__ uint32_t pos(uint32_t q, uint32_t gene) const { return gene_begin[q] + (gene - N); }
    __device__ uint32_t task(uint32_t q, uint32_t) const { return q; }
    __device__ uint32_t cm_at(uint32_t q) const { return gene_begin[q]; }
    __device__ uint32_t genome(uint32_t gene) const { return gene < N ? genome_b[gene] : G; }
};

// list j = edges [edge_begin[j], edge_begin[j + 1]) in ids [0, N + n_query[j]); d_bad = n_queries - (the first failing query)
__global__ __launch_bounds__(256) void k_place_check_batch(const int32_t *src, const int32_t *dst, const uint64_t *edge_begin, const uint32_t *n_query, uint32_t nq,
                                                           uint32_t N, unsigned long long *d_bad) {
    const uint64_t E = edge_begin[nq];
    for (uint64_t e = (uint64_t) blockIdx.x * 256 + threadIdx.x; e < E; e += (uint64_t) gridDim.x * 256) {
        const uint32_t j = last_le(edge_begin, nq, e);
        const uint32_t NC = N + n_query[j];
        const uint32_t a = (uint32_t) src[e], b = (uint32_t) dst[e];                 // (a negative id is a large unsigned one)
        if (a >= NC || b >= NC || (a < N && b < N)) atomicMax(d_bad, (unsigned long long) (nq - j));
    }
}

// The layout of the queries of a chunk ([nq + 1] each on the device; the last entry closes the list)
struct PlaceChunk {
    const uint32_t *gene_begin;       // first chunk gene of query q
    const uint32_t *shift;            // flat id of query q's own id 0
    const uint32_t *edge_begin;       // first edge of query q in the edge list the launch works on
    uint32_t nq, N;
    static constexpr const char *too_large = "K-place: 2^31 ids or edges and more in one chunk of the batch (option query_batch_bytes cuts smaller chunks)";
    static void lists(pdl_ctx *c, const PlaceQueries &Q, uint32_t N, PlaceChunk L[2]) {
        const uint32_t n1 = Q.nq + 1;
        c->pb.blay.alloc((size_t) 4 * n1 * 4);
        uint32_t *d = c->pb.blay.as<uint32_t>();
        const std::vector<uint32_t> *h[4] = {&Q.gene_begin, &Q.shift, &Q.eb[0], &Q.eb[1]};
        for (int i = 0; i < 4; i++) PDL_HIP(hipMemcpyAsync(d + i * n1, h[i]->data(), (size_t) n1 * 4, hipMemcpyHostToDevice, c->stream));
        for (int l = 0; l < 2; l++) L[l] = PlaceChunk{d, d + n1, d + (2 + l) * n1, Q.nq, N};
    }
    __device__ uint32_t query_of_edge(uint32_t e) const { return last_le(edge_begin, nq, e); }
    __device__ uint32_t query_of_gene(uint32_t g) const { return last_le(gene_begin, nq, g); }
    __device__ uint32_t query_of_flat(uint32_t f) const { return last_le(shift, nq, f); }
    __device__ uint32_t flat(uint32_t q, uint32_t x) const { return shift[q] + x; }
    __device__ uint32_t gene(uint32_t q, uint32_t x) const { return gene_begin[q] + (x - N); }         // chunk gene of the own id x >= N
};

static uint64_t *place_batch_begin(pdl_ctx *c) {
    (void) place_begin(c);
    c->pb.bctl.alloc(PDL_PB_WORDS * sizeof(uint64_t));
    PDL_HIP(hipMemsetAsync(c->pb.bctl.p, 0, PDL_PB_WORDS * sizeof(uint64_t), c->stream));
    return c->pb.bctl.as<uint64_t>();
}

// One chunk behind its device half: K-bbh over all its cells, then the placement stages over all its edges; the placements go to out[qa..).
static void place_chunk(pdl_ctx *c, const PlaceBase &B, const std::vector<QBQuery> &qs, uint32_t qa, const pdl_query_cells &ch,
                        std::vector<pdl_place_result> &out, pdl_query_info *info, float *device_ms) {
    hipStream_t st = c->stream;
    pdl_ctx::PlaceBufs &b = c->pb;
    const uint32_t N = c->N, nq = ch.nq, NT = ch.genes;
    const uint64_t Z = ch.Z;
    if (Z >= 0x7fffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "more than 2^31 cells in one chunk of the query batch (option query_batch_bytes cuts smaller chunks)");
    std::vector<uint32_t> h_cb(nq + 1, 0);
    for (uint32_t q = 0; q < nq; q++) {
        if (h_cb[q] + ch.cells_of[q] > Z) PDL_FAIL(PDL_ERR_DEVICE, "place batch: the queries' cells pass the emitted total %llu", (unsigned long long) Z);
        h_cb[q + 1] = h_cb[q] + (uint32_t) ch.cells_of[q];
    }
    if (h_cb[nq] != Z) PDL_FAIL(PDL_ERR_DEVICE, "place batch: the queries' cells (%u) are not the emitted total %llu", h_cb[nq], (unsigned long long) Z);
    uint64_t *d_tot = place_batch_begin(c) + PDL_PB_EDGES_1;
    std::vector<uint64_t> e1(nq + 1, 0), e2(nq + 1, 0);             // first phase-1 / phase-2 edge of every query
    uint8_t *h_edges[6] = {};                                       // the chunk's edges on the host: src, dst, score of phase 1, then of phase 2
    BbhEdges e{};
    b.bspans.start(st);
    if (Z) {                                                       // P-bbh: a block and a task per query
        b.bspans.begin();
        const float *cf = ch.cells;
        e = bbh_edges(c, cf, reinterpret_cast<const int32_t *>(cf + 3 * ch.cap), reinterpret_cast<const int32_t *>(cf + 4 * ch.cap),
                      [&](const uint32_t *d_cb) { return BbhQueryChunk{c->d_gen, ch.d_gene_begin, d_cb, N, c->G, nq}; },
                      ch.MS, ch.CM, N, c->G + 1, nq, NT, Z, b.bbh, d_tot, h_cb.data(), nq);
        b.bspans.end();
        bbh_read_counts(c, "place batch", d_tot, e, h_cb.data(), nq, Z, qa, e1, e2);
        // the edges themselves: the chunk's in one piece per array, into the batch's pinned staging; they are cut out once the
        // placement stages have waited for the stream
        const uint64_t n[2] = {e1[nq], e2[nq]};
        c->qbb.stage.alloc((size_t) (n[0] + n[1]) * 12);
        bbh_copy_out(st, e, n, h_edges, c->qbb.stage.p);
    }
    // P-cc .. P-out once over the chunk
    PlaceQueries Q;
    Q.nq = nq;
    for (uint32_t q = 0; q < nq; q++) Q.n.push_back(qs[qa + q].n);
    Q.lay_out(N);
    Q.eb[0].assign(e1.begin(), e1.end()); Q.eb[1].assign(e2.begin(), e2.end());
    b.spans.start(st);
    b.spans.begin();
    const float place_ms = place_run<PlaceChunk>(c, B, Q, e.src, e.dst, true, false, b.spans, &out[qa]);
    for (uint32_t q = 0; q < nq; q++) {
        pdl_place_result &r = out[qa + q];
        const uint64_t ne[2] = {e1[q + 1] - e1[q], e2[q + 1] - e2[q]};
        uint8_t *h[6];                                              // its edges, cut out of the staging in one pass
        place_c_edges(r, ne, h);
        for (int i = 0; i < 6; i++)
            if (ne[i / 3]) memcpy(h[i], h_edges[i] + (i < 3 ? e1[q] : e2[q]) * 4, ne[i / 3] * 4);
    }
    // (place_run has waited for the stream: the chunk's events have all been reached)
    const float query_ms = ch.device_ms(), total_ms = query_ms + b.bspans.total_ms() + place_ms;
    *device_ms += total_ms;
    for (uint32_t q = 0; q < nq; q++) {
        out[qa + q].device_ms = total_ms / (float) nq;
        if (info) ch.info_of(q, qs[qa + q].Rq, qs[qa + q].Mq, query_ms / (float) nq, &info[qa + q]);
    }
}

// pdl_place_batch behind its refusals of state and argument: the families of the context are valid (c->fam).  Nothing is handed
// out before the last chunk is through: a refusal found in a later chunk leaves `out` to its owner.
void pdl_run_place_batch(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, const uint32_t *gene_begin, uint32_t n, uint32_t n_queries,
                         std::vector<pdl_place_result> &out, pdl_query_info *info, uint32_t *chunks, float *device_ms) {
    out.clear();
    out.resize(n_queries);
    const PlaceBase B = place_context_base(c);
    std::vector<QBQuery> qs;
    const uint32_t hbm_cols = pdl_query_batch_plan(c, offsets, gene_begin, n, n_queries, qs, 8);      // (parent and grp_of_label: 4 bytes each per flat id)
    *chunks = 0; *device_ms = 0.f;
    for (uint32_t qa = 0; qa < n_queries;) {
        uint32_t qe = pdl_query_batch_chunk_end(c, qs, qa);
        uint64_t genes = 0;
        for (uint32_t q = qa; q < qe; q++) {                         // ... cut where the flat ids would reach 2^31 (a chunk of one always fits)
            genes += qs[q].n;
            if (q > qa && place_flat_ids(c->N, q - qa + 1, genes) >= 0x7fffffffull) { qe = q; break; }
        }
        const pdl_query_cells ch = pdl_run_query_chunk_device(c, residues, offsets, qs, qa, qe, hbm_cols);       // (its argument and domain refusals leave from here)
        place_chunk(c, B, qs, qa, ch, out, info, device_ms);
        (*chunks)++;
        qa += ch.nq;                                                 // (option "query_rekey" may have cut the chunk short of qe)
    }
}

// pdl_placement_batch_of_edges behind its argument checks: the lists end to end on the device, edge_begin [n_queries + 1] from 0
void pdl_run_place_batch_edges(pdl_ctx *c, const PlaceBase &base, uint32_t n_queries, const uint32_t *n_query, const uint64_t *edge_begin,
                               const int32_t *d_src, const int32_t *d_dst, std::vector<pdl_place_result> &out) {
    hipStream_t st = c->stream;
    pdl_ctx::PlaceBufs &b = c->pb;
    out.clear();
    out.resize(n_queries);
    uint64_t *bctl = place_batch_begin(c);
    const uint64_t E = edge_begin[n_queries];
    if (E) {                                                       // PB-check
        b.up_edge_begin.alloc(((size_t) n_queries + 1) * 8); b.up_n_query.alloc((size_t) n_queries * 4);
        PDL_HIP(hipMemcpyAsync(b.up_edge_begin.p, edge_begin, ((size_t) n_queries + 1) * 8, hipMemcpyHostToDevice, st));
        PDL_HIP(hipMemcpyAsync(b.up_n_query.p, n_query, (size_t) n_queries * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_place_check_batch, dim3((uint32_t) std::min<uint64_t>((E + 255) / 256, 4096)), dim3(256), 0, st, d_src, d_dst,
                           (const uint64_t *) b.up_edge_begin.as<uint64_t>(), (const uint32_t *) b.up_n_query.as<uint32_t>(), n_queries, base.N,
                           reinterpret_cast<unsigned long long *>(bctl + PDL_PB_BAD_QUERY));
        const uint64_t bad = pdl_gate(c, bctl + PDL_PB_BAD_QUERY);
        if (bad) {
            const uint32_t j = n_queries - (uint32_t) bad;
            PDL_FAIL(PDL_ERR_ARGUMENT, "K-place: query %u: its edges name a gene id outside [0, %u) or join two base genes (ids below %u)", j, base.N + n_query[j], base.N);
        }
    }
    // runs of consecutive queries whose flat ids and edges stay below 2^31 (one query always fits: checked by the caller)
    for (uint32_t qa = 0; qa < n_queries;) {
        uint32_t qe = qa;
        uint64_t genes = 0;
        while (qe < n_queries && (qe == qa || (place_flat_ids(base.N, qe - qa + 1, genes + n_query[qe]) < 0x7fffffffull && edge_begin[qe + 1] - edge_begin[qa] < 0x7fffffffull)))
            genes += n_query[qe++];
        PlaceQueries Q;
        Q.nq = qe - qa;
        Q.n.assign(n_query + qa, n_query + qe);
        Q.lay_out(base.N);
        Q.eb[0].resize(Q.nq + 1); Q.eb[1].assign(Q.nq + 1, 0);
        for (uint32_t q = qa; q <= qe; q++) Q.eb[0][q - qa] = (uint32_t) (edge_begin[q] - edge_begin[qa]);
        (void) place_begin(c);
        b.spans.start(st);
        b.spans.begin();
        const int32_t *src[2] = {d_src + edge_begin[qa], nullptr}, *dst[2] = {d_dst + edge_begin[qa], nullptr};
        const float ms = place_run<PlaceChunk>(c, base, Q, src, dst, false, true, b.spans, &out[qa]);
        for (uint32_t q = qa; q < qe; q++) out[q].device_ms = ms / (float) Q.nq;
        qa = qe;
    }
}
