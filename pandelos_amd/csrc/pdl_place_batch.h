// pdl_place_batch.h — K-place for a batch: q new genomes placed into the gene families that are already built, each on its own
// (pdl_place_batch, pdl_placement_batch_of_edges; included from pdl_bbh.hip behind pdl_place.h).
//
// Contract: placement j is what pdl_place_query returns for genome j alone — ids are query j's own union ids (its genes are
// N..N+n_j-1 of genome G).  The queries never see each other; the base context is only read.
//
// Per chunk of the query batch (pdl_query_batch.h cuts the chunks), on one stream, no cell crosses PCIe; the stages of
// place_run (pdl_place.h) run ONCE over the chunk with the query folded into the ids:
//
//   B-alpha .. B-order   pdl_run_query_chunk_device: the chunk's ordered cells, MS and CM stay in c->qbb, query after query
//   PB-bbh     k_bbh_mark/_threshold/_intra (pdl_bbh.hip) over all cells of the chunk with BbhQueryChunk: a cell's row is an id
//              of its own query's union, so the query comes from the cell's index against the per-query cell offsets; MS row =
//              gene_begin[q] + (row - N), the CM slice at q * N + gene_begin[q], inter_max [q][G + 1], thr [chunk gene].  The two
//              kinds compacted in cell order over the chunk (KindFlag / EdgeApply): a query's phase-1 and phase-2 edges are one
//              stretch each, its counts the prefixes at its first cell (k_pick_prefixes); one PinRead
//   PB-check   k_place_check_batch (callers' lists only): every list against its OWN [0, N + n_q) and for base-base edges, in one
//              launch, before any id indexes anything; the first failing query leaves by an atomicMax
//   PB-cc      union-find over flat ids: query q's own id x is shift[q] + x, shift[q] = q * N + gene_begin[q] — the queries'
//              unions [N + n_q] one behind the other, as the CM slices lie.  k_pb_init: every query's copy of the base's
//              component_of, moved by shift[q]; its genes identity.  parent[x] <= x holds from the start, so fam_union / fam_find
//              are K-fam's and a tree's root is its query's smallest own id: its smallest base label, or its smallest query gene.
//              k_pb_union maps an edge's ends through its query (the edge's index against the per-query edge offsets);
//              k_pb_roots: the flat root of every chunk gene and the sort key of PB-groups
//   PB-degree  same_deg over chunk genes: phase 2's distinct pairs (k_pb_intra), or callers' lists compacted to (lo, hi) keys of
//              chunk genes, sorted and counted at the run heads (k_fam_intra_sorted)
//   PB-groups  pdl_sort_pairs (flat root, chunk gene), run heads + scan (FamHeadFlag / FamHeadApply): groups in (query, label)
//              order — a query's groups are one stretch —, their members ascending, the chunk-wide group index of every flat label
//   PB-base    edges with a base end -> (chunk-wide group, base label) keys (PBBaseApply), then P-base's functors and kernels as
//   PB-bridge  they are: a group belongs to one query, so (group, base label) and (group, genome) keys keep the queries apart
//   PB-clique  k_place_clique over the sorted chunk genes
//   PB-out     one PinRead of the chunk's counts (the member total sizes PB-bridge), then the arrays come over whole and the
//              placements are cut out and translated to each query's own ids on the host
//
// The per-query copies of the base's labels and the label-indexed group table take 8 (N + n_q) bytes per query; a chunk is cut
// where its flat ids would reach 2^31 (a chunk of one always fits).
#pragma once

#include "pdl_place.h"

// the queries of a chunk: `part` = the query of cell i (the last q with cell_begin[q] <= i: empty queries lie before it)
struct BbhQueryChunk {
    const uint32_t *genome_b, *gene_begin, *cell_begin; uint32_t N, G, nq;
    __device__ uint32_t part(uint32_t i) const {
        uint32_t lo = 0, hi = nq;
        while (hi - lo > 1) { const uint32_t m = (lo + hi) >> 1; if (cell_begin[m] <= i) lo = m; else hi = m; }
        return lo;
    }
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
        uint32_t lo = 0, hi = nq;                                 // last list j with edge_begin[j] <= e (empty lists lie before it)
        while (hi - lo > 1) { const uint32_t m = (lo + hi) >> 1; if (edge_begin[m] <= e) lo = m; else hi = m; }
        const uint32_t NC = N + n_query[lo];
        const uint32_t a = (uint32_t) src[e], b = (uint32_t) dst[e];                 // (a negative id is a large unsigned one)
        if (a >= NC || b >= NC || (a < N && b < N)) atomicMax(d_bad, (unsigned long long) (nq - lo));
    }
}

// The queries of a chunk as the kernels below find them ([nq + 1] each; the last entry closes the list)
struct PBLayout {
    const uint32_t *gene_begin;       // first chunk gene of query q
    const uint32_t *shift;            // flat id of query q's own id 0: q * N + gene_begin[q]
    const uint32_t *edge_begin;       // first edge of query q in the edge list the launch works on
    uint32_t nq, N;
    static __device__ uint32_t last_le(const uint32_t *at, uint32_t n, uint32_t v) {      // last q with at[q] <= v (empty stretches lie before it)
        uint32_t lo = 0, hi = n;
        while (hi - lo > 1) { const uint32_t m = (lo + hi) >> 1; if (at[m] <= v) lo = m; else hi = m; }
        return lo;
    }
    __device__ uint32_t query_of_edge(uint32_t e) const { return last_le(edge_begin, nq, e); }
    __device__ uint32_t query_of_gene(uint32_t g) const { return last_le(gene_begin, nq, g); }
    __device__ uint32_t query_of_flat(uint32_t f) const { return last_le(shift, nq, f); }
    __device__ uint32_t flat(uint32_t q, uint32_t x) const { return shift[q] + x; }
    __device__ uint32_t gene(uint32_t q, uint32_t x) const { return gene_begin[q] + (x - N); }         // chunk gene of the own id x >= N
};

__global__ __launch_bounds__(256) void k_pb_init(PBLayout L, const uint32_t *comp, uint32_t F, uint32_t NT, uint32_t *parent, uint32_t *same_deg, uint8_t *is_node,
                                                 uint8_t *gcol) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < F) {
        const uint32_t s = L.shift[L.query_of_flat(i)], x = i - s;
        parent[i] = x < L.N ? s + comp[x] : i;
    }
    if (i < NT) { same_deg[i] = 0; is_node[i] = 0; gcol[i] = 0; }
}
// as k_place_union, an edge's ends mapped through its query; is_node by chunk gene
__global__ __launch_bounds__(256) void k_pb_union(const int32_t *src, const int32_t *dst, uint32_t n_edges, uint32_t mirrored, PBLayout L, uint32_t *parent,
                                                  uint8_t *is_node) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const uint32_t a = (uint32_t) src[e], b = (uint32_t) dst[e];
    if (mirrored && a > b) return;
    const uint32_t q = L.query_of_edge(e);
    if (a >= L.N) is_node[L.gene(q, a)] = 1;
    if (b >= L.N) is_node[L.gene(q, b)] = 1;
    if (a != b) fam_union(parent, L.flat(q, a), L.flat(q, b));
}
// phase 2 (list 1): distinct query-query pairs
__global__ __launch_bounds__(256) void k_pb_intra(const int32_t *src, const int32_t *dst, uint32_t n_edges, PBLayout L, uint32_t *same_deg) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const uint32_t a = (uint32_t) src[e], b = (uint32_t) dst[e];
    if (a == b || a < L.N || b < L.N) return;
    const uint32_t q = L.query_of_edge(e);
    atomicAdd(same_deg + L.gene(q, a), 1u); atomicAdd(same_deg + L.gene(q, b), 1u);
}
// callers' lists: a query-query edge (PlaceIntraFlag) as the (lo << 32 | hi) key of its two chunk genes
struct PBIntraApply {
    const int32_t *src, *dst; PBLayout L; unsigned long long *keys;
    __device__ void operator()(uint64_t e, uint32_t f, uint32_t pre) const {
        if (!f) return;
        const uint32_t q = L.query_of_edge((uint32_t) e);
        const uint32_t a = L.gene(q, (uint32_t) src[e]), b = L.gene(q, (uint32_t) dst[e]);
        keys[pre] = (unsigned long long) (a < b ? a : b) << 32 | (a < b ? b : a);
    }
};
// family[g] = the flat root of chunk gene g (its own flat id when it is no node); key[g] = the sort key of PB-groups (`F` behind all)
__global__ __launch_bounds__(256) void k_pb_roots(uint32_t *parent, const uint8_t *is_node, PBLayout L, uint32_t F, uint32_t NT, uint32_t *family, uint32_t *key) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= NT) return;
    const uint32_t q = L.query_of_gene(g), f = L.flat(q, L.N + (g - L.gene_begin[q]));
    const uint32_t r = is_node[g] ? fam_find(parent, f) : f;
    family[g] = r;
    key[g] = is_node[g] ? r : F;
}
// an edge with one base end (PlaceBaseFlag) as the key (chunk-wide group << label_bits | base label)
struct PBBaseApply {
    const int32_t *src, *dst; PBLayout L; uint32_t label_bits;
    const uint32_t *family, *grp_of_label, *base_comp; unsigned long long *keys;
    __device__ void operator()(uint64_t e, uint32_t f, uint32_t pre) const {
        if (!f) return;
        const uint32_t a = (uint32_t) src[e], b = (uint32_t) dst[e];
        const uint32_t qg = a < L.N ? b : a, g = a < L.N ? a : b;
        keys[pre] = (unsigned long long) grp_of_label[family[L.gene(L.query_of_edge((uint32_t) e), qg)]] << label_bits | base_comp[g];
    }
};

// The layout of nq queries for one run of the batched stages: n[q] genes each, the edges of query q at eb[l][q] .. eb[l][q + 1] of list l
struct PBQueries {
    uint32_t nq = 0;
    std::vector<uint32_t> n, gene_begin, shift, eb[2];            // [nq], then [nq + 1] each
    void lay_out(uint32_t N) {
        gene_begin.assign(nq + 1, 0); shift.assign(nq + 1, 0);
        for (uint32_t q = 0; q < nq; q++) gene_begin[q + 1] = gene_begin[q] + n[q];
        for (uint32_t q = 0; q <= nq; q++) shift[q] = q * N + gene_begin[q];
    }
};
// flat ids a run over these queries would take (a run needs them below 2^31)
static inline uint64_t pb_flat_ids(uint32_t N, uint64_t nq, uint64_t genes) { return nq * N + genes; }

// The stages of place_run once over nq queries.  list[0] / list[1]: device edge lists, every query's edges one stretch (Q.eb), in
// the query's own union ids; mirrored0 / caller as place_run's (a caller's ids have been checked).  `spans` has a stretch open on
// entry and none on return.  -> out[0 .. nq): every field but the edges and device_ms; returns the device time of its stretches.
// The twin of place_run (pdl_place.h), stage for stage: the sorts, scans, count checks and the bridge stage are the same calls
// over the chunk's sizes — a change to one belongs into the other.  (place_run is this with nq = 1 and shift = 0, without the
// searches for an edge's query.)
static float place_run_batch(pdl_ctx *c, const PlaceBase &B, const PBQueries &Q, const int32_t *const src[2], const int32_t *const dst[2], bool mirrored0,
                             bool caller, QSpans &spans, pdl_place_result *out) {
    hipStream_t st = c->stream;
    pdl_ctx::PlaceBufs &b = c->pb;
    const uint32_t N = B.N, nq = Q.nq, NT = Q.gene_begin[nq];
    const uint64_t n_edges[2] = {Q.eb[0][nq], Q.eb[1][nq]};
    if (pb_flat_ids(N, nq, NT) >= 0x7fffffffull || n_edges[0] >= 0x7fffffffull || n_edges[1] >= 0x7fffffffull)
        PDL_FAIL(PDL_ERR_UNSUPPORTED, "K-place: 2^31 ids or edges and more in one chunk of the batch (option query_batch_bytes cuts smaller chunks)");
    const uint32_t F = Q.shift[nq];
    uint64_t *ctl = b.ctl.as<uint64_t>();
    const size_t n4 = (size_t) NT * 4, L4 = ((size_t) nq + 1) * 4;
    b.parent.alloc((size_t) F * 4); b.grp_of_label.alloc((size_t) F * 4);
    b.is_node.alloc(NT); b.gcol.alloc(NT); b.same_deg.alloc(n4); b.family_of.alloc(n4); b.gq_off.alloc(n4 + 4); b.gb_off.alloc(n4 + 4);
    for (DevBuf *d : {&b.mk_a, &b.mk_b, &b.mv_a, &b.mv_b}) d->alloc(n4);
    b.blay.alloc(4 * L4);
    uint32_t *parent = b.parent.as<uint32_t>(), *same_deg = b.same_deg.as<uint32_t>(), *family = b.family_of.as<uint32_t>();
    uint32_t *grp_of_label = b.grp_of_label.as<uint32_t>(), *gq_off = b.gq_off.as<uint32_t>(), *gb_off = b.gb_off.as<uint32_t>();
    uint8_t *is_node = b.is_node.as<uint8_t>(), *gcol = b.gcol.as<uint8_t>();
    uint32_t *d_lay = b.blay.as<uint32_t>();
    PDL_HIP(hipMemcpyAsync(d_lay, Q.gene_begin.data(), L4, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(d_lay + (nq + 1), Q.shift.data(), L4, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(d_lay + 2 * (nq + 1), Q.eb[0].data(), L4, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(d_lay + 3 * (nq + 1), Q.eb[1].data(), L4, hipMemcpyHostToDevice, st));
    const PBLayout L{d_lay, d_lay + (nq + 1), d_lay + 2 * (nq + 1), nq, N};            // (over list 0)
    const PBLayout L1{d_lay, d_lay + (nq + 1), d_lay + 3 * (nq + 1), nq, N};          // (over list 1)
    // PB-cc
    hipLaunchKernelGGL(k_pb_init, fam_grid(F), dim3(256), 0, st, L, B.comp, F, NT, parent, same_deg, is_node, gcol);
    for (int l = 0; l < 2; l++)
        if (n_edges[l]) hipLaunchKernelGGL(k_pb_union, fam_grid(n_edges[l]), dim3(256), 0, st, src[l], dst[l], (uint32_t) n_edges[l], (uint32_t) (l == 0 && mirrored0), l ? L1 : L, parent, is_node);
    uint32_t *mk_in = b.mk_a.as<uint32_t>(), *mk_out = b.mk_b.as<uint32_t>(), *mv_in = b.mv_a.as<uint32_t>(), *mv_out = b.mv_b.as<uint32_t>();
    hipLaunchKernelGGL(k_pb_roots, fam_grid(NT), dim3(256), 0, st, parent, (const uint8_t *) is_node, L, F, NT, family, mk_in);
    PDL_HIP(hipGetLastError());
    // PB-degree
    const uint64_t E0 = n_edges[0];
    if (caller) {
        if (E0) {
            b.ek_a.alloc(E0 * 8); b.ek_b.alloc(E0 * 8); b.ev_a.alloc(E0 * 4); b.ev_b.alloc(E0 * 4);
            unsigned long long *ek_in = b.ek_a.as<unsigned long long>();
            uint32_t *ev_in = b.ev_a.as<uint32_t>(), *ev_out = b.ev_b.as<uint32_t>();
            uint64_t *d_intra = ctl + PDL_PL_INTRA;
            scan_and_apply(c, E0, PlaceIntraFlag{src[0], dst[0], N}, PBIntraApply{src[0], dst[0], L, ek_in}, d_intra);
            uint64_t *k_in = reinterpret_cast<uint64_t *>(ek_in), *k_out = b.ek_b.as<uint64_t>();
            pdl_sort_pairs<uint64_t, uint32_t>(c, k_in, k_out, ev_in, ev_out, E0, 32 + bit_length64(NT - 1), true, d_intra, 0, true);
            hipLaunchKernelGGL(k_fam_intra_sorted, fam_grid(E0), dim3(256), 0, st, reinterpret_cast<const unsigned long long *>(k_out), d_intra, same_deg, 0u);
        }
    } else if (n_edges[1]) {
        hipLaunchKernelGGL(k_pb_intra, fam_grid(n_edges[1]), dim3(256), 0, st, src[1], dst[1], (uint32_t) n_edges[1], L1, same_deg);
    }
    PDL_HIP(hipGetLastError());
    // PB-groups: (flat root, chunk gene), chunk genes ascending in
    pdl_sort_pairs<uint32_t, uint32_t>(c, mk_in, mk_out, mv_in, mv_out, NT, bit_length64(F), true, nullptr, 0, true);
    scan_and_apply(c, NT, FamHeadFlag{mk_out, mv_out, nullptr, F}, FamHeadApply{mk_out, nullptr, F, NT, gq_off, grp_of_label, ctl + PDL_PL_NODES}, ctl + PDL_PL_GROUPS);
    // PB-base
    const uint32_t label_bits = std::max<uint32_t>(1, bit_length64(N ? N - 1 : 0)), group_bits = std::max<uint32_t>(1, bit_length64(NT));
    const uint32_t genome_bits = std::max<uint32_t>(1, bit_length64(B.G));
    unsigned long long *uniq = nullptr;
    uint32_t *group_base = nullptr, *mpre = nullptr;
    if (E0) {
        b.bk_a.alloc(E0 * 8); b.bk_b.alloc(E0 * 8); b.bv_a.alloc(E0 * 4); b.bv_b.alloc(E0 * 4); b.uniq.alloc(E0 * 8); b.group_base.alloc(E0 * 4); b.mpre.alloc(E0 * 4);
        uniq = b.uniq.as<unsigned long long>(); group_base = b.group_base.as<uint32_t>(); mpre = b.mpre.as<uint32_t>();
        uint64_t *k_in = b.bk_a.as<uint64_t>(), *k_out = b.bk_b.as<uint64_t>();
        uint32_t *v_in = b.bv_a.as<uint32_t>(), *v_out = b.bv_b.as<uint32_t>();
        uint64_t *d_base = ctl + PDL_PL_BASE_EDGES, *d_pairs = ctl + PDL_PL_BASE_PAIRS;
        scan_and_apply(c, E0, PlaceBaseFlag{src[0], dst[0], (uint32_t) mirrored0, N},
                       PBBaseApply{src[0], dst[0], L, label_bits, family, grp_of_label, B.comp, reinterpret_cast<unsigned long long *>(k_in)}, d_base);
        pdl_sort_pairs<uint64_t, uint32_t>(c, k_in, k_out, v_in, v_out, E0, label_bits + group_bits, true, d_base, 0, true);
        const unsigned long long *sorted = reinterpret_cast<const unsigned long long *>(k_out);
        scan_and_apply(c, E0, PlaceUniqFlag{sorted}, PlaceUniqApply{sorted, uniq, group_base, gcol, B, label_bits}, d_pairs, nullptr, d_base);
        hipLaunchKernelGGL(k_place_base_off, fam_grid((uint64_t) NT + 1), dim3(256), 0, st, uniq, d_pairs, ctl + PDL_PL_GROUPS, NT, label_bits, gb_off);
        scan_and_apply(c, E0, PlaceMemberFlag{uniq, gb_off, B, label_bits}, PlaceMemberApply{mpre}, ctl + PDL_PL_MEMBERS, nullptr, d_pairs);
    }
    // PB-clique
    hipLaunchKernelGGL(k_place_clique, fam_grid(NT), dim3(256), 0, st, mk_out, mv_out, grp_of_label, gq_off, same_deg, ctl + PDL_PL_NODES, NT, gcol);
    PDL_HIP(hipGetLastError());
    spans.end();
    // PB-out: the chunk's counts in one read ...
    uint64_t nodes, groups, pairs, members;
    {
        PinRead rd(c);
        const uint64_t *w = rd.add<uint64_t>(ctl + PDL_PL_NODES, PDL_PL_MEMBERS - PDL_PL_NODES + 1);
        rd.sync();
        nodes = w[PDL_PL_NODES - PDL_PL_NODES]; groups = w[PDL_PL_GROUPS - PDL_PL_NODES]; pairs = w[PDL_PL_BASE_PAIRS - PDL_PL_NODES]; members = w[PDL_PL_MEMBERS - PDL_PL_NODES];
    }
    if (nodes > NT || groups > nodes || pairs > E0 || (groups == 0 && pairs) || members >= 0x7fffffffull)
        PDL_FAIL(PDL_ERR_DEVICE, "K-place: inconsistent counts (%llu nodes, %llu groups, %llu base pairs, %llu members of %u query genes, %llu edges)",
                 (unsigned long long) nodes, (unsigned long long) groups, (unsigned long long) pairs, (unsigned long long) members, NT, (unsigned long long) E0);
    // ... PB-bridge, sized by the member total ...
    if (members) {
        spans.begin();
        b.bk_a.alloc(members * 8); b.bk_b.alloc(members * 8); b.bv_a.alloc(members * 4); b.bv_b.alloc(members * 4);
        uint64_t *k_in = b.bk_a.as<uint64_t>(), *k_out = b.bk_b.as<uint64_t>();
        uint32_t *v_in = b.bv_a.as<uint32_t>(), *v_out = b.bv_b.as<uint32_t>();
        hipLaunchKernelGGL(k_place_gather, fam_grid(members), dim3(256), 0, st, uniq, mpre, (uint32_t) pairs, (uint32_t) members, B, label_bits, genome_bits,
                           reinterpret_cast<unsigned long long *>(k_in), v_in);
        pdl_sort_pairs<uint64_t, uint32_t>(c, k_in, k_out, v_in, v_out, members, genome_bits + group_bits, false, nullptr, 0, true);
        hipLaunchKernelGGL(k_place_bridge, fam_grid(members), dim3(256), 0, st, reinterpret_cast<const unsigned long long *>(k_out), v_out, (uint32_t) members, genome_bits, gcol);
        PDL_HIP(hipGetLastError());
        spans.end();
    }
    // ... then the arrays, whole
    std::vector<uint32_t> h_family(NT), h_gq_off(groups + 1, 0), h_gb_off(groups + 1, 0), h_gene(nodes), h_base(pairs);
    std::vector<uint8_t> h_is_node(NT), h_gcol(groups);
    PDL_HIP(hipMemcpyAsync(h_family.data(), family, n4, hipMemcpyDeviceToHost, st));
    PDL_HIP(hipMemcpyAsync(h_is_node.data(), is_node, NT, hipMemcpyDeviceToHost, st));
    if (groups) {
        PDL_HIP(hipMemcpyAsync(h_gq_off.data(), gq_off, (groups + 1) * 4, hipMemcpyDeviceToHost, st));
        PDL_HIP(hipMemcpyAsync(h_gene.data(), mv_out, nodes * 4, hipMemcpyDeviceToHost, st));
        PDL_HIP(hipMemcpyAsync(h_gcol.data(), gcol, groups, hipMemcpyDeviceToHost, st));
        if (E0) PDL_HIP(hipMemcpyAsync(h_gb_off.data(), gb_off, (groups + 1) * 4, hipMemcpyDeviceToHost, st));
        if (pairs) PDL_HIP(hipMemcpyAsync(h_base.data(), group_base, pairs * 4, hipMemcpyDeviceToHost, st));
    }
    PDL_HIP(hipStreamSynchronize(st));
    if (groups && (h_gq_off[0] != 0 || h_gq_off[groups] != nodes || h_gb_off[groups] != pairs)) PDL_FAIL(PDL_ERR_DEVICE, "K-place: inconsistent group offsets");
    for (uint64_t g = 0; g < groups; g++)
        if (h_gq_off[g + 1] <= h_gq_off[g] || h_gq_off[g + 1] > nodes || h_gb_off[g + 1] < h_gb_off[g] || h_gb_off[g + 1] > pairs || h_gene[h_gq_off[g]] >= NT)
            PDL_FAIL(PDL_ERR_DEVICE, "K-place: inconsistent group members");
    // every query's placement cut out: its groups are one stretch (a group is its first member's query's), ids back in its own union
    uint64_t g = 0;
    for (uint32_t q = 0; q < nq; q++) {
        pdl_place_result &r = out[q];
        const uint32_t n = Q.n[q], g0 = Q.gene_begin[q], s = Q.shift[q];
        r.sequences = N; r.n_query = n; r.genomes = B.G;
        r.family_of.resize(n); r.is_node.assign(h_is_node.begin() + g0, h_is_node.begin() + g0 + n);
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t f = h_family[g0 + i];
            if (f < s || f > s + N + i) PDL_FAIL(PDL_ERR_DEVICE, "K-place: a family label outside its query's ids");
            r.family_of[i] = f - s;
        }
        const uint64_t ga = g;
        while (g < groups && h_gene[h_gq_off[g]] < g0 + n) {
            if (h_gene[h_gq_off[g]] < g0) PDL_FAIL(PDL_ERR_DEVICE, "K-place: the groups are not in the queries' order");
            g++;
        }
        const uint32_t ng = (uint32_t) (g - ga), m0 = ng ? h_gq_off[ga] : 0, p0 = ng ? h_gb_off[ga] : 0;
        r.groups = ng;
        r.group_query_off.assign(ng + 1, 0); r.group_base_off.assign(ng + 1, 0); r.group_label.resize(ng); r.group_collides.resize(ng);
        for (uint32_t j = 0; j <= ng; j++) { r.group_query_off[j] = h_gq_off[ga + j] - m0; r.group_base_off[j] = h_gb_off[ga + j] - p0; }
        if (!ng) { r.group_query_off[0] = 0; r.group_base_off[0] = 0; }
        const uint32_t nodes_q = r.group_query_off[ng];
        r.group_query.resize(nodes_q);
        for (uint32_t j = 0; j < nodes_q; j++) {
            const uint32_t cg = h_gene[m0 + j];
            if (cg < g0 || cg >= g0 + n) PDL_FAIL(PDL_ERR_DEVICE, "K-place: a group with members of two queries");
            r.group_query[j] = N + (cg - g0);
        }
        r.group_base.assign(h_base.begin() + p0, h_base.begin() + p0 + r.group_base_off[ng]);
        r.unplaced = n - nodes_q;
        for (uint32_t j = 0; j < ng; j++) {
            const uint32_t nb = r.group_base_off[j + 1] - r.group_base_off[j];
            r.group_label[j] = r.family_of[r.group_query[r.group_query_off[j]] - N];
            r.group_collides[j] = h_gcol[ga + j];
            (nb == 0 ? r.novel : nb == 1 ? r.joined : r.bridging)++;
            r.colliding += r.group_collides[j] ? 1u : 0u;
        }
    }
    if (g != groups) PDL_FAIL(PDL_ERR_DEVICE, "K-place: groups behind the last query");
    return spans.total_ms();
}

static uint64_t *place_batch_begin(pdl_ctx *c) {
    (void) place_begin(c);
    c->pb.bctl.alloc(PDL_PB_WORDS * sizeof(uint64_t));
    PDL_HIP(hipMemsetAsync(c->pb.bctl.p, 0, PDL_PB_WORDS * sizeof(uint64_t), c->stream));
    return c->pb.bctl.as<uint64_t>();
}

// One chunk behind its device half: K-bbh over all its cells, then the placement stages over all its edges; the placements go to out[qa..).
static void place_chunk(pdl_ctx *c, const PlaceBase &B, const std::vector<QBQuery> &qs, uint32_t qa, const pdl_query_chunk &ch,
                        std::vector<pdl_place_result> &out, pdl_query_info *info, float *device_ms) {
    hipStream_t st = c->stream;
    pdl_ctx::PlaceBufs &b = c->pb;
    const uint32_t N = c->N, G1 = c->G + 1, nq = ch.nq, NT = ch.genes;
    const uint64_t Z = ch.Z;
    if (Z >= 0x7fffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "more than 2^31 cells in one chunk of the query batch (option query_batch_bytes cuts smaller chunks)");
    std::vector<uint32_t> h_cb(nq + 1, 0);
    for (uint32_t q = 0; q < nq; q++) {
        if (h_cb[q] + ch.cells[q] > Z) PDL_FAIL(PDL_ERR_DEVICE, "place batch: the queries' cells pass the emitted total %llu", (unsigned long long) Z);
        h_cb[q + 1] = h_cb[q] + (uint32_t) ch.cells[q];
    }
    if (h_cb[nq] != Z) PDL_FAIL(PDL_ERR_DEVICE, "place batch: the queries' cells (%u) are not the emitted total %llu", h_cb[nq], (unsigned long long) Z);
    uint64_t *bctl = place_batch_begin(c);
    std::vector<uint64_t> e1(nq + 1, 0), e2(nq + 1, 0);             // first phase-1 / phase-2 edge of every query
    uint8_t *h_edges[6] = {};                                       // the chunk's edges on the host: src, dst, score of phase 1, then of phase 2
    int32_t *src1 = nullptr, *dst1 = nullptr, *src2 = nullptr, *dst2 = nullptr;
    b.bspans.start(st);
    if (Z) {                                                       // PB-bbh
        b.bspans.begin();
        b.kind.alloc(Z + 16);
        b.tab.alloc(((size_t) nq * G1 + NT + 2 * (Z + 1)) * sizeof(uint32_t));
        b.btab.alloc(3 * ((size_t) nq + 1) * sizeof(uint32_t));
        uint32_t *inter_max = b.tab.as<uint32_t>(), *thr = inter_max + (size_t) nq * G1, *pre1 = thr + NT, *pre2 = pre1 + (Z + 1);
        uint32_t *d_cb = b.btab.as<uint32_t>(), *d_pick = d_cb + (nq + 1);
        PDL_HIP(hipMemcpyAsync(d_cb, h_cb.data(), ((size_t) nq + 1) * 4, hipMemcpyHostToDevice, st));
        PDL_HIP(hipMemsetAsync(inter_max, 0, (size_t) nq * G1 * sizeof(uint32_t), st));
        hipLaunchKernelGGL(k_fill_u32, dim3((NT + 255) / 256), dim3(256), 0, st, thr, NT, 0x7f800000u);
        const float *cf = c->qbb.cells.as<float>();
        BbhArgs<BbhQueryChunk> a{};
        a.score = cf; a.row = reinterpret_cast<const int32_t *>(cf + 3 * ch.cap); a.col = reinterpret_cast<const int32_t *>(cf + 4 * ch.cap);
        a.at = BbhQueryChunk{c->d_gen, c->qbb.gene_begin.as<uint32_t>(), d_cb, N, c->G, nq};
        a.MS = c->qbb.MS.as<float>(); a.CM = c->qbb.CM.as<float>(); a.N = N; a.G = G1; a.Z = (uint32_t) Z;      // (a.N: what a query's CM slice starts at a multiple of)
        a.inter_max = inter_max; a.thr = thr; a.kind = b.kind.as<uint8_t>();
        bbh_filter(st, a);
        b.e_src.alloc(3 * Z * sizeof(int32_t)); b.e_dst.alloc(3 * Z * sizeof(int32_t)); b.e_score.alloc(3 * Z * sizeof(float));
        src1 = b.e_src.as<int32_t>(); dst1 = b.e_dst.as<int32_t>();
        float *sc1 = b.e_score.as<float>(), *sc2 = sc1 + 2 * Z;
        src2 = src1 + 2 * Z; dst2 = dst1 + 2 * Z;
        scan_and_apply(c, Z, KindFlag{a.kind, 1}, EdgeApply{a.score, a.row, a.col, src1, dst1, sc1, pre1, 2}, bctl + PDL_PB_EDGES_1);
        scan_and_apply(c, Z, KindFlag{a.kind, 2}, EdgeApply{a.score, a.row, a.col, src2, dst2, sc2, pre2, 1}, bctl + PDL_PB_EDGES_2);
        // cells of each kind before every query: the prefixes at its first cell (the totals close the lists)
        hipLaunchKernelGGL(k_pick_prefixes, dim3((nq + 1 + 255) / 256), dim3(256), 0, st, pre1, pre2, d_cb, nq + 1, (uint32_t) Z, d_pick);
        PDL_HIP(hipGetLastError());
        b.bspans.end();
        uint64_t n1, n2;
        {
            PinRead rd(c);
            const uint64_t *pt = rd.add<uint64_t>(bctl + PDL_PB_EDGES_1, PDL_PB_EDGES_2 - PDL_PB_EDGES_1 + 1);
            const uint32_t *pp = rd.add<uint32_t>(d_pick, 2 * ((size_t) nq + 1));
            rd.sync();
            const uint64_t t1 = pt[PDL_PB_EDGES_1 - PDL_PB_EDGES_1], t2 = pt[PDL_PB_EDGES_2 - PDL_PB_EDGES_1];
            if (t1 > Z || t2 > Z) PDL_FAIL(PDL_ERR_DEVICE, "place batch: %llu + %llu edge cells of %llu cells", (unsigned long long) t1, (unsigned long long) t2, (unsigned long long) Z);
            for (uint32_t q = 0; q <= nq; q++) {
                const bool past = h_cb[q] >= Z;
                e1[q] = 2 * (past ? t1 : (uint64_t) pp[q]); e2[q] = past ? t2 : (uint64_t) pp[nq + 1 + q];
            }
            n1 = 2 * t1; n2 = t2;
        }
        for (uint32_t q = 0; q < nq; q++)
            if (e1[q + 1] < e1[q] || e2[q + 1] < e2[q] || e1[q + 1] > n1 || e2[q + 1] > n2) PDL_FAIL(PDL_ERR_DEVICE, "place batch: inconsistent edge offsets at query %u", qa + q);
        // the edges themselves: the chunk's in one piece per array, into the batch's pinned staging (a DMA, no staging by the
        // runtime and no page of a fresh vector to touch); they are cut out once the placement stages have waited for the stream
        const size_t stage_bytes = (size_t) (n1 + n2) * 12;
        auto &w = c->qbb;
        if (w.stage_bytes < stage_bytes) {
            if (w.stage) { (void) hipHostFree(w.stage); w.stage = nullptr; w.stage_bytes = 0; }
            PDL_HIP(hipHostMalloc((void **) &w.stage, stage_bytes + stage_bytes / 4, hipHostMallocDefault));
            w.stage_bytes = stage_bytes + stage_bytes / 4;
        }
        uint8_t *m = w.stage;                // layout: src1 | dst1 | sc1 | src2 | dst2 | sc2
        h_edges[0] = m; h_edges[1] = m + n1 * 4; h_edges[2] = m + n1 * 8; h_edges[3] = m + n1 * 12; h_edges[4] = m + n1 * 12 + n2 * 4; h_edges[5] = m + n1 * 12 + n2 * 8;
        if (n1) {
            PDL_HIP(hipMemcpyAsync(h_edges[0], src1, n1 * 4, hipMemcpyDeviceToHost, st));
            PDL_HIP(hipMemcpyAsync(h_edges[1], dst1, n1 * 4, hipMemcpyDeviceToHost, st));
            PDL_HIP(hipMemcpyAsync(h_edges[2], sc1, n1 * 4, hipMemcpyDeviceToHost, st));
        }
        if (n2) {
            PDL_HIP(hipMemcpyAsync(h_edges[3], src2, n2 * 4, hipMemcpyDeviceToHost, st));
            PDL_HIP(hipMemcpyAsync(h_edges[4], dst2, n2 * 4, hipMemcpyDeviceToHost, st));
            PDL_HIP(hipMemcpyAsync(h_edges[5], sc2, n2 * 4, hipMemcpyDeviceToHost, st));
        }
    }
    // PB-cc .. PB-out once over the chunk
    PBQueries Q;
    Q.nq = nq;
    for (uint32_t q = 0; q < nq; q++) Q.n.push_back(qs[qa + q].n);
    Q.lay_out(N);
    Q.eb[0].assign(e1.begin(), e1.end()); Q.eb[1].assign(e2.begin(), e2.end());
    b.spans.start(st);
    b.spans.begin();
    const int32_t *src[2] = {src1, src2}, *dst[2] = {dst1, dst2};
    const float place_ms = place_run_batch(c, B, Q, src, dst, true, false, b.spans, &out[qa]);
    for (uint32_t q = 0; q < nq; q++) {
        pdl_place_result &r = out[qa + q];
        const uint64_t ne[2] = {e1[q + 1] - e1[q], e2[q + 1] - e2[q]};
        // its edges as the C arrays the caller gets, in the host's insertion order: phase 1, then phase 2 — one pass out of the staging
        pdl_place_result::CEdges &ce = r.c_edges;
        ce.drop();
        ce.n = ne[0] + ne[1]; ce.set = true;
        const size_t bytes = std::max<size_t>(ce.n, 1) * 4;
        ce.src = static_cast<int32_t *>(malloc(bytes)); ce.dst = static_cast<int32_t *>(malloc(bytes)); ce.score = static_cast<float *>(malloc(bytes));
        if (!ce.src || !ce.dst || !ce.score) throw std::bad_alloc();
        uint64_t at_out = 0;
        for (int l = 0; l < 2; l++) {
            if (!ne[l]) continue;
            const uint64_t at = l ? e2[q] : e1[q];
            memcpy(ce.src + at_out, h_edges[3 * l] + at * 4, ne[l] * 4);
            memcpy(ce.dst + at_out, h_edges[3 * l + 1] + at * 4, ne[l] * 4);
            memcpy(ce.score + at_out, h_edges[3 * l + 2] + at * 4, ne[l] * 4);
            at_out += ne[l];
        }
        r.edges_phase1 = (uint32_t) ne[0];
    }
    // (place_run_batch has waited for the stream: the chunk's events have all been reached)
    const float query_ms = c->qbb.spans.total_ms(), total_ms = query_ms + b.bspans.total_ms() + place_ms;
    *device_ms += total_ms;
    for (uint32_t q = 0; q < nq; q++) {
        out[qa + q].device_ms = total_ms / (float) nq;
        if (info) {
            const QBQuery &one = qs[qa + q];
            pdl_query_info &fi = info[qa + q];
            memset(&fi, 0, sizeof(fi));
            fi.residues = one.Rq; fi.kmer_occurrences = one.Mq; fi.records = ch.records[q]; fi.matched_records = ch.matched[q];
            fi.genome_cost = ch.cost[q];
            fi.device_ms = query_ms / (float) nq;
        }
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
            if (q > qa && pb_flat_ids(c->N, q - qa + 1, genes) >= 0x7fffffffull) { qe = q; break; }
        }
        const pdl_query_chunk ch = pdl_run_query_chunk_device(c, residues, offsets, qs, qa, qe, hbm_cols);       // (its argument and domain refusals leave from here)
        place_chunk(c, B, qs, qa, ch, out, info, device_ms);
        (*chunks)++;
        qa = qe;
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
        PDL_HIP(hipGetLastError());
        PinRead rd(c);
        const uint64_t *bad = rd.add<uint64_t>(bctl + PDL_PB_BAD_QUERY, 1);
        rd.sync();
        if (*bad) {
            const uint32_t j = n_queries - (uint32_t) *bad;
            PDL_FAIL(PDL_ERR_ARGUMENT, "K-place: query %u: its edges name a gene id outside [0, %u) or join two base genes (ids below %u)", j, base.N + n_query[j], base.N);
        }
    }
    // runs of consecutive queries whose flat ids and edges stay below 2^31 (one query always fits: checked by the caller)
    for (uint32_t qa = 0; qa < n_queries;) {
        uint32_t qe = qa;
        uint64_t genes = 0;
        while (qe < n_queries && (qe == qa || (pb_flat_ids(base.N, qe - qa + 1, genes + n_query[qe]) < 0x7fffffffull && edge_begin[qe + 1] - edge_begin[qa] < 0x7fffffffull)))
            genes += n_query[qe++];
        PBQueries Q;
        Q.nq = qe - qa;
        Q.n.assign(n_query + qa, n_query + qe);
        Q.lay_out(base.N);
        Q.eb[0].resize(Q.nq + 1); Q.eb[1].assign(Q.nq + 1, 0);
        for (uint32_t q = qa; q <= qe; q++) Q.eb[0][q - qa] = (uint32_t) (edge_begin[q] - edge_begin[qa]);
        (void) place_begin(c);
        b.spans.start(st);
        b.spans.begin();
        const int32_t *src[2] = {d_src + edge_begin[qa], nullptr}, *dst[2] = {d_dst + edge_begin[qa], nullptr};
        const float ms = place_run_batch(c, base, Q, src, dst, false, true, b.spans, &out[qa]);
        for (uint32_t q = qa; q < qe; q++) out[q].device_ms = ms / (float) Q.nq;
        qa = qe;
    }
}
