// pdl_place.h — K-place: new genomes' genes placed into the gene families that are already built (pdl_place_query,
// pdl_placement_of_edges, and through pdl_place_batch.h their batch forms; included from pdl_bbh.hip behind pdl_families.h).
// A query's Scores block (K-query, pdl_query.h) is filtered where it lies — K-bbh's three kernels — and the edges are hung onto
// the base network's components without clustering the base again: the union-find of K-fam starts from the base's labels.
//
// A query's ids are its union ids: base genes 0..N-1, its genes N..N+n-1 (genome G).  Every edge has a query end; a base-base edge
// is refused.  One run (place_run) takes nq queries that never see each other.  It works on flat ids (query q's own id x is
// flat(q, x)) and chunk genes (the queries' genes one behind the other); how an edge, a gene or a flat id finds its query is the
// layout's business, a template parameter of the run and of the kernels that map ids.  PlaceOne is a single query: one query 0,
// flat(0, x) = x, gene x - N, constants to the compiler and nothing on the device.  PlaceChunk (pdl_place_batch.h) is a chunk
// of a batch.
//
//   P-bbh      bbh_edges (pdl_bbh.hip): k_bbh_mark/_threshold/_intra with the caller's locator (BbhQueryBlock: row p = gene - N, one
//              task, genome G for ids >= N) over K-place's own BbhBufs; the two kinds compacted in cell order (KindFlag /
//              EdgeApply): phase 1 ((row, col) then (col, row)), phase 2.  bbh_read_counts brings the totals, bbh_copy_out the edges
//   P-check    k_place_check    (a caller's list only, by its entry point) ids outside [0, N + n) and base-base edges counted; read
//              BEFORE anything below
//   P-cc       k_place_init: every query's copy of the base's component_of moved to its flat ids (the only O(N) step), its genes
//              identity: parent[x] <= x holds from the start, so fam_union / fam_find (pdl_families.h) over the edges leave every
//              tree's root its smallest member.  k_place_union marks the query genes that are a node; k_place_roots: the flat
//              root of every chunk gene and the sort keys
//   P-degree   same_deg of the chunk genes from the query-query edges: phase 2's distinct pairs (k_place_intra), or a caller's list
//              compacted to (lo, hi) keys of chunk genes, sorted and counted at the run heads (k_fam_intra_sorted)
//   P-groups   pdl_sort_pairs (flat root, chunk gene), run heads + scan (FamHeadFlag / FamHeadApply): groups in (query, label)
//              order — a query's groups are one stretch —, their members ascending, the group index of every flat label
//   P-base     edges with a base end -> (group, base label) keys, compacted, sorted, run heads: every group's fused base components;
//              a component that collides in the base flags its group (a lookup)
//   P-bridge   groups of two or more base components: their members gathered (a gene that was no node is its own), keyed by
//              (group, genome), sorted; a run with genes of two components flags the group — such genes cannot be adjacent, every
//              new edge has a query end.  A group belongs to one query, so both keys keep the queries apart
//   P-clique   a group's m >= 2 query genes are clean exactly when each has same_deg == m - 1 (as F-collide)
//   P-out      one PinRead of the counts (the member total sizes P-bridge), then the arrays come over whole; every query's
//              placement is cut out of them and translated to its own ids on the host
//
// Work: the queries' edges plus the members of bridged components; of the work nothing but the parent init is proportional to N.
// Memory is: parent and grp_of_label (indexed by flat label, touched at the groups' labels only) hold N + n words per query.
#pragma once

#include "pdl_common.h"
#include "pdl_scan.h"
#include "pdl_sort.h"

// the one task of a query block: MS [n][G + 1], CM [N + n], inter_max [G + 1], thr [n]
struct BbhQueryBlock {
    const uint32_t *genome_b; uint32_t N, G;
    __device__ uint32_t part(uint32_t) const { return 0u; }
    __device__ uint32_t pos(uint32_t, uint32_t gene) const { return gene - N; }
    __device__ uint32_t task(uint32_t, uint32_t) const { return 0u; }
    __device__ uint32_t cm_at(uint32_t) const { return 0u; }
    __device__ uint32_t genome(uint32_t gene) const { return gene < N ? genome_b[gene] : G; }
};

// The queries of one run: n[q] genes each, the edges of query q at eb[l][q] .. eb[l][q + 1] of list l.  Query q's own id x is the
// flat id shift[q] + x, shift[q] = q * N + gene_begin[q]: the queries' unions [N + n_q] one behind the other
struct PlaceQueries {
    uint32_t nq = 0;
    std::vector<uint32_t> n, gene_begin, shift, eb[2];            // [nq], then [nq + 1] each
    void lay_out(uint32_t N) {
        gene_begin.assign(nq + 1, 0); shift.assign(nq + 1, 0);
        for (uint32_t q = 0; q < nq; q++) gene_begin[q + 1] = gene_begin[q] + n[q];
        for (uint32_t q = 0; q <= nq; q++) shift[q] = q * N + gene_begin[q];
    }
    static PlaceQueries one(uint32_t N, uint32_t n, uint64_t e0, uint64_t e1) {
        PlaceQueries Q;
        Q.nq = 1; Q.n = {n};
        Q.lay_out(N);
        Q.eb[0] = {0u, (uint32_t) e0}; Q.eb[1] = {0u, (uint32_t) e1};
        return Q;
    }
};
// flat ids a run over nq queries would take (a run needs them below 2^31)
static inline uint64_t place_flat_ids(uint32_t N, uint64_t nq, uint64_t genes) { return nq * N + genes; }

// The layout of a single query: its union ids are the flat ids.  (`lists`: the layouts over list 0 and list 1 of a run.)
struct PlaceOne {
    uint32_t N;
    static constexpr const char *too_large = "K-place: 2^31 genes or edges and more";
    static void lists(pdl_ctx *, const PlaceQueries &, uint32_t N, PlaceOne L[2]) { L[0] = L[1] = PlaceOne{N}; }
    __device__ uint32_t query_of_edge(uint32_t) const { return 0u; }
    __device__ uint32_t query_of_gene(uint32_t) const { return 0u; }
    __device__ uint32_t query_of_flat(uint32_t) const { return 0u; }
    __device__ uint32_t flat(uint32_t, uint32_t x) const { return x; }
    __device__ uint32_t gene(uint32_t, uint32_t x) const { return x - N; }            // chunk gene of the own id x >= N
};

// parent of every flat id: a base gene's label moved to its query's flat ids, a query gene its own; the chunk genes' arrays cleared
template <class Lay>
__global__ __launch_bounds__(256) void k_place_init(Lay L, const uint32_t *comp, uint32_t F, uint32_t NT, uint32_t *parent, uint32_t *same_deg, uint8_t *is_node,
                                                    uint8_t *gcol) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < F) {
        const uint32_t s = L.flat(L.query_of_flat(i), 0), x = i - s;
        parent[i] = x < L.N ? s + comp[x] : i;
    }
    if (i < NT) { same_deg[i] = 0; is_node[i] = 0; gcol[i] = 0; }
}
__global__ __launch_bounds__(256) void k_place_check(const int32_t *src, const int32_t *dst, uint32_t n_edges, uint32_t N, uint32_t NC, uint64_t *d_bad) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const uint32_t a = (uint32_t) src[e], b = (uint32_t) dst[e];                 // (a negative id is a large unsigned one)
    if (a >= NC || b >= NC || (a < N && b < N)) atomicAdd(reinterpret_cast<unsigned long long *>(d_bad), 1ull);
}
// as k_fam_union, an edge's ends mapped through its query; only the query genes' node flags are kept, by chunk gene
template <class Lay>
__global__ __launch_bounds__(256) void k_place_union(const int32_t *src, const int32_t *dst, uint32_t n_edges, uint32_t mirrored, Lay L, uint32_t *parent,
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
template <class Lay>
__global__ __launch_bounds__(256) void k_place_intra(const int32_t *src, const int32_t *dst, uint32_t n_edges, Lay L, uint32_t *same_deg) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const uint32_t a = (uint32_t) src[e], b = (uint32_t) dst[e];
    if (a == b || a < L.N || b < L.N) return;
    const uint32_t q = L.query_of_edge(e);
    atomicAdd(same_deg + L.gene(q, a), 1u); atomicAdd(same_deg + L.gene(q, b), 1u);
}
// a caller's list: a query-query edge ...
struct PlaceIntraFlag {
    const int32_t *src, *dst; uint32_t N;
    __device__ uint32_t operator()(uint64_t e) const { const uint32_t a = (uint32_t) src[e], b = (uint32_t) dst[e]; return (uint32_t) (a != b && a >= N && b >= N); }
};
// ... as the (lo << 32 | hi) key of its two chunk genes
template <class Lay>
struct PlaceIntraApply {
    const int32_t *src, *dst; Lay L; unsigned long long *keys;
    __device__ void operator()(uint64_t e, uint32_t f, uint32_t pre) const {
        if (!f) return;
        const uint32_t q = L.query_of_edge((uint32_t) e);
        const uint32_t a = L.gene(q, (uint32_t) src[e]), b = L.gene(q, (uint32_t) dst[e]);
        keys[pre] = (unsigned long long) (a < b ? a : b) << 32 | (a < b ? b : a);
    }
};
// family[g] = the flat root of chunk gene g (its own flat id when it is no node); key[g] = the sort key of P-groups (`F` behind all)
template <class Lay>
__global__ __launch_bounds__(256) void k_place_roots(uint32_t *parent, const uint8_t *is_node, Lay L, uint32_t F, uint32_t NT, uint32_t *family, uint32_t *key) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= NT) return;
    const uint32_t q = L.query_of_gene(g), f = L.flat(q, L.N + (g - L.gene(q, L.N)));
    const uint32_t r = is_node[g] ? fam_find(parent, f) : f;
    family[g] = r;
    key[g] = is_node[g] ? r : F;
}

// an edge with one base end (a mirrored list holds it twice: the half with src < dst is taken) ...
struct PlaceBaseFlag {
    const int32_t *src, *dst; uint32_t mirrored, N;
    __device__ uint32_t operator()(uint64_t e) const {
        const uint32_t a = (uint32_t) src[e], b = (uint32_t) dst[e];
        if (mirrored && a > b) return 0u;
        return (uint32_t) ((a < N) != (b < N));
    }
};
// ... as the key (group << label_bits | base label)
template <class Lay>
struct PlaceBaseApply {
    const int32_t *src, *dst; Lay L; uint32_t label_bits;
    const uint32_t *family, *grp_of_label, *base_comp; unsigned long long *keys;
    __device__ void operator()(uint64_t e, uint32_t f, uint32_t pre) const {
        if (!f) return;
        const uint32_t a = (uint32_t) src[e], b = (uint32_t) dst[e];
        const uint32_t qg = a < L.N ? b : a, g = a < L.N ? a : b;
        keys[pre] = (unsigned long long) grp_of_label[family[L.gene(L.query_of_edge((uint32_t) e), qg)]] << label_bits | base_comp[g];
    }
};
// run heads of the sorted keys: the distinct (group, base component) pairs; a component that collides in the base flags its group
struct PlaceUniqFlag {
    const unsigned long long *keys;
    __device__ uint32_t operator()(uint64_t j) const { return (uint32_t) (j == 0 || keys[j - 1] != keys[j]); }
};
struct PlaceUniqApply {
    const unsigned long long *keys; unsigned long long *uniq; uint32_t *group_base; uint8_t *gcol; PlaceBase B; uint32_t label_bits;
    __device__ void operator()(uint64_t j, uint32_t f, uint32_t pre) const {
        if (!f) return;
        const unsigned long long k = keys[j];
        const uint32_t label = (uint32_t) (k & ((1ull << label_bits) - 1));
        uniq[pre] = k; group_base[pre] = label;
        if (B.is_node[label] && B.collides[B.fam_of_label[label]]) gcol[k >> label_bits] = 1;
    }
};
// gb_off[g] = first pair of group g, for g = 0..groups
__global__ __launch_bounds__(256) void k_place_base_off(const unsigned long long *uniq, const uint64_t *d_pairs, const uint64_t *d_groups, uint32_t n, uint32_t label_bits,
                                                        uint32_t *gb_off) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g > n || g > *d_groups) return;
    const unsigned long long want = (unsigned long long) g << label_bits;
    uint32_t lo = 0, hi = (uint32_t) *d_pairs;
    while (lo < hi) { const uint32_t m = lo + ((hi - lo) >> 1); if (uniq[m] < want) lo = m + 1; else hi = m; }
    gb_off[g] = lo;
}
// members a pair brings to P-bridge: the component's genes when its group fuses two or more, else none
struct PlaceMemberFlag {
    const unsigned long long *uniq; const uint32_t *gb_off; PlaceBase B; uint32_t label_bits;
    __device__ uint32_t operator()(uint64_t j) const {
        const unsigned long long k = uniq[j];
        const uint32_t g = (uint32_t) (k >> label_bits), label = (uint32_t) (k & ((1ull << label_bits) - 1));
        if (gb_off[g + 1] - gb_off[g] < 2) return 0u;
        if (!B.is_node[label]) return 1u;
        const uint32_t f = B.fam_of_label[label];
        return B.fam_off[f + 1] - B.fam_off[f];
    }
};
struct PlaceMemberApply {
    uint32_t *mpre;
    __device__ void operator()(uint64_t j, uint32_t, uint32_t pre) const { mpre[j] = pre; }
};
// member t of the gathered list -> key (group << genome_bits | genome), value = its base component
__global__ __launch_bounds__(256) void k_place_gather(const unsigned long long *uniq, const uint32_t *mpre, uint32_t pairs, uint32_t members, PlaceBase B, uint32_t label_bits,
                                                      uint32_t genome_bits, unsigned long long *key, uint32_t *val) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= members) return;
    uint32_t lo = 0, hi = pairs;                      // last pair j with mpre[j] <= t: the one that holds member t (pairs without members share their successor's prefix)
    while (hi - lo > 1) { const uint32_t m = (lo + hi) >> 1; if (mpre[m] <= t) lo = m; else hi = m; }
    const unsigned long long k = uniq[lo];
    const uint32_t g = (uint32_t) (k >> label_bits), label = (uint32_t) (k & ((1ull << label_bits) - 1));
    const uint32_t gene = B.is_node[label] ? B.fam_genes[B.fam_off[B.fam_of_label[label]] + (t - mpre[lo])] : label;
    key[t] = (unsigned long long) g << genome_bits | B.genome_of[gene];
    val[t] = label;
}
__global__ __launch_bounds__(256) void k_place_bridge(const unsigned long long *key, const uint32_t *val, uint32_t members, uint32_t genome_bits, uint8_t *gcol) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t == 0 || t >= members) return;
    if (key[t] == key[t - 1] && val[t] != val[t - 1]) gcol[key[t] >> genome_bits] = 1;
}
// position j of the sorted (root, query gene) list
__global__ __launch_bounds__(256) void k_place_clique(const uint32_t *key, const uint32_t *gene, const uint32_t *grp_of_label, const uint32_t *gq_off, const uint32_t *same_deg,
                                                      const uint64_t *d_nodes, uint32_t n, uint8_t *gcol) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n || j >= *d_nodes) return;
    const uint32_t g = grp_of_label[key[j]], m = gq_off[g + 1] - gq_off[g];
    if (m >= 2 && same_deg[gene[j]] != m - 1) gcol[g] = 1;
}

static uint64_t *place_begin(pdl_ctx *c) {
    pdl_ctl_ready(c);
    c->pb.ctl.alloc(PDL_PL_WORDS * sizeof(uint64_t));
    PDL_HIP(hipMemsetAsync(c->pb.ctl.p, 0, PDL_PL_WORDS * sizeof(uint64_t), c->stream));
    return c->pb.ctl.as<uint64_t>();
}

// The placement stages once over the nq queries of Q.  list[0] / list[1]: device edge lists, every query's edges one stretch (Q.eb),
// in the query's own union ids (the query blocks' two phases, or callers' lists and nothing).  mirrored0: list 0 holds every pair in
// both directions.  caller: query-query edges (looked for in list 0) may repeat; otherwise they are list 1's, distinct.  A caller's
// ids have been checked.  `spans` has a stretch open on entry and none on return.  -> out[0 .. nq): every field but the edges and
// device_ms; returns the device time of its stretches.
template <class Lay>
static float place_run(pdl_ctx *c, const PlaceBase &B, const PlaceQueries &Q, const int32_t *const src[2], const int32_t *const dst[2], bool mirrored0,
                       bool caller, QSpans &spans, pdl_place_result *out) {
    hipStream_t st = c->stream;
    pdl_ctx::PlaceBufs &b = c->pb;
    const uint32_t N = B.N, nq = Q.nq, NT = Q.gene_begin[nq];
    const uint64_t n_edges[2] = {Q.eb[0][nq], Q.eb[1][nq]};
    if (place_flat_ids(N, nq, NT) >= 0x7fffffffull || n_edges[0] >= 0x7fffffffull || n_edges[1] >= 0x7fffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "%s", Lay::too_large);
    const uint32_t F = Q.shift[nq];
    uint64_t *ctl = b.ctl.as<uint64_t>();
    const size_t n4 = (size_t) NT * 4;
    b.parent.alloc((size_t) F * 4); b.grp_of_label.alloc((size_t) F * 4);
    b.is_node.alloc(NT); b.gcol.alloc(NT); b.same_deg.alloc(n4); b.family_of.alloc(n4); b.gq_off.alloc(n4 + 4); b.gb_off.alloc(n4 + 4);
    for (DevBuf *d : {&b.mk_a, &b.mk_b, &b.mv_a, &b.mv_b}) d->alloc(n4);
    uint32_t *parent = b.parent.as<uint32_t>(), *same_deg = b.same_deg.as<uint32_t>(), *family = b.family_of.as<uint32_t>();
    uint32_t *grp_of_label = b.grp_of_label.as<uint32_t>(), *gq_off = b.gq_off.as<uint32_t>(), *gb_off = b.gb_off.as<uint32_t>();
    uint8_t *is_node = b.is_node.as<uint8_t>(), *gcol = b.gcol.as<uint8_t>();
    Lay lay[2];                                       // (over list 0, over list 1)
    Lay::lists(c, Q, N, lay);
    const Lay &L = lay[0];
    // P-cc
    hipLaunchKernelGGL(k_place_init<Lay>, grid256(F), dim3(256), 0, st, L, B.comp, F, NT, parent, same_deg, is_node, gcol);
    for (int l = 0; l < 2; l++)
        if (n_edges[l]) hipLaunchKernelGGL(k_place_union<Lay>, grid256(n_edges[l]), dim3(256), 0, st, src[l], dst[l], (uint32_t) n_edges[l], (uint32_t) (l == 0 && mirrored0), lay[l], parent, is_node);
    uint32_t *mk_in = b.mk_a.as<uint32_t>(), *mk_out = b.mk_b.as<uint32_t>(), *mv_in = b.mv_a.as<uint32_t>(), *mv_out = b.mv_b.as<uint32_t>();
    hipLaunchKernelGGL(k_place_roots<Lay>, grid256(NT), dim3(256), 0, st, parent, (const uint8_t *) is_node, L, F, NT, family, mk_in);
    PDL_HIP(hipGetLastError());
    // P-degree
    const uint64_t E0 = n_edges[0];
    if (caller) {
        if (E0) {
            b.ek_a.alloc(E0 * 8); b.ek_b.alloc(E0 * 8); b.ev_a.alloc(E0 * 4); b.ev_b.alloc(E0 * 4);
            unsigned long long *ek_in = b.ek_a.as<unsigned long long>();
            uint32_t *ev_in = b.ev_a.as<uint32_t>(), *ev_out = b.ev_b.as<uint32_t>();
            uint64_t *d_intra = ctl + PDL_PL_INTRA;
            scan_and_apply(c, E0, PlaceIntraFlag{src[0], dst[0], N}, PlaceIntraApply<Lay>{src[0], dst[0], L, ek_in}, d_intra);
            uint64_t *k_in = reinterpret_cast<uint64_t *>(ek_in), *k_out = b.ek_b.as<uint64_t>();
            pdl_sort_pairs<uint64_t, uint32_t>(c, k_in, k_out, ev_in, ev_out, E0, 32 + bit_length64(NT - 1), true, d_intra, 0, true);
            hipLaunchKernelGGL(k_fam_intra_sorted, grid256(E0), dim3(256), 0, st, reinterpret_cast<const unsigned long long *>(k_out), d_intra, same_deg, 0u);
        }
    } else if (n_edges[1]) {
        hipLaunchKernelGGL(k_place_intra<Lay>, grid256(n_edges[1]), dim3(256), 0, st, src[1], dst[1], (uint32_t) n_edges[1], lay[1], same_deg);
    }
    PDL_HIP(hipGetLastError());
    // P-groups: (flat root, chunk gene), chunk genes ascending in
    pdl_sort_pairs<uint32_t, uint32_t>(c, mk_in, mk_out, mv_in, mv_out, NT, bit_length64(F), true, nullptr, 0, true);
    scan_and_apply(c, NT, FamHeadFlag{mk_out, mv_out, nullptr, F}, FamHeadApply{mk_out, nullptr, F, NT, gq_off, grp_of_label, ctl + PDL_PL_NODES}, ctl + PDL_PL_GROUPS);
    // P-base
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
                       PlaceBaseApply<Lay>{src[0], dst[0], L, label_bits, family, grp_of_label, B.comp, reinterpret_cast<unsigned long long *>(k_in)}, d_base);
        pdl_sort_pairs<uint64_t, uint32_t>(c, k_in, k_out, v_in, v_out, E0, label_bits + group_bits, true, d_base, 0, true);
        const unsigned long long *sorted = reinterpret_cast<const unsigned long long *>(k_out);
        scan_and_apply(c, E0, PlaceUniqFlag{sorted}, PlaceUniqApply{sorted, uniq, group_base, gcol, B, label_bits}, d_pairs, nullptr, d_base);
        hipLaunchKernelGGL(k_place_base_off, grid256((uint64_t) NT + 1), dim3(256), 0, st, uniq, d_pairs, ctl + PDL_PL_GROUPS, NT, label_bits, gb_off);
        scan_and_apply(c, E0, PlaceMemberFlag{uniq, gb_off, B, label_bits}, PlaceMemberApply{mpre}, ctl + PDL_PL_MEMBERS, nullptr, d_pairs);
    }
    // P-clique
    hipLaunchKernelGGL(k_place_clique, grid256(NT), dim3(256), 0, st, mk_out, mv_out, grp_of_label, gq_off, same_deg, ctl + PDL_PL_NODES, NT, gcol);
    PDL_HIP(hipGetLastError());
    spans.end();
    // P-out: the counts in one read ...
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
    // ... P-bridge, sized by the member total ...
    if (members) {
        spans.begin();
        b.bk_a.alloc(members * 8); b.bk_b.alloc(members * 8); b.bv_a.alloc(members * 4); b.bv_b.alloc(members * 4);
        uint64_t *k_in = b.bk_a.as<uint64_t>(), *k_out = b.bk_b.as<uint64_t>();
        uint32_t *v_in = b.bv_a.as<uint32_t>(), *v_out = b.bv_b.as<uint32_t>();
        hipLaunchKernelGGL(k_place_gather, grid256(members), dim3(256), 0, st, uniq, mpre, (uint32_t) pairs, (uint32_t) members, B, label_bits, genome_bits,
                           reinterpret_cast<unsigned long long *>(k_in), v_in);
        pdl_sort_pairs<uint64_t, uint32_t>(c, k_in, k_out, v_in, v_out, members, genome_bits + group_bits, false, nullptr, 0, true);
        hipLaunchKernelGGL(k_place_bridge, grid256(members), dim3(256), 0, st, reinterpret_cast<const unsigned long long *>(k_out), v_out, (uint32_t) members, genome_bits, gcol);
        PDL_HIP(hipGetLastError());
        spans.end();
    }
    // ... then the arrays, whole
    std::vector<uint32_t> h_family(NT), h_gq_off(groups + 1, 0), h_gb_off(groups + 1, 0), h_gene(nodes), h_base(pairs);
    std::vector<uint8_t> h_is_node(NT), h_gcol(groups);
    copy_down(st, h_family, family, NT); copy_down(st, h_is_node, is_node, NT);
    if (groups) {
        copy_down(st, h_gq_off, gq_off, groups + 1); copy_down(st, h_gene, mv_out, nodes); copy_down(st, h_gcol, gcol, groups);
        if (E0) copy_down(st, h_gb_off, gb_off, groups + 1);
        copy_down(st, h_base, group_base, pairs);
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

// A base network's families (host view f) on their way to the device, into `b`: the six arrays queued on the stream, of_label
// derived on the host and kept in b while its copy is under way.  -> the device view, with the caller's genome ids (on the device)
PlaceBase pdl_upload_base(pdl_ctx *c, const FamView &f, BaseBufs &b, const uint32_t *d_genome_of, uint32_t G) {
    hipStream_t st = c->stream;
    const size_t N = f.N, F = f.families, nodes = f.nodes;
    fam_of_label(f, b.of_label);
    b.comp.alloc(N * 4); b.is_node.alloc(N); b.fam_of_label.alloc(N * 4); b.fam_off.alloc((F + 1) * 4); b.fam_genes.alloc(nodes * 4); b.collides.alloc(F);
    const struct { DevBuf &d; const void *h; size_t bytes; } up[6] = {{b.comp, f.component_of, N * 4}, {b.is_node, f.is_node, N}, {b.fam_of_label, b.of_label.data(), N * 4},
                                                                      {b.fam_off, f.family_off, (F + 1) * 4}, {b.fam_genes, f.family_genes, nodes * 4}, {b.collides, f.collides, F}};
    for (const auto &u : up)
        if (u.bytes) PDL_HIP(hipMemcpyAsync(u.d.p, u.h, u.bytes, hipMemcpyHostToDevice, st));
    return b.view(f.N, d_genome_of, G);
}

// the context's own families on the device: uploaded once per run of K-fam (c->fam is its answer on the host)
static PlaceBase place_context_base(pdl_ctx *c) {
    pdl_ctx::PlaceBufs &b = c->pb;
    const pdl_fam_result &f = c->fam;
    const uint32_t N = c->N;
    if (f.sequences != N || f.component_of.size() != N) PDL_FAIL(PDL_ERR_STATE, "K-place: the context's families are not those of its %u genes", N);
    if (b.base_serial != c->fam_serial) {
        b.base_serial = 0;
        pdl_upload_base(c, FamView{N, f.families, f.nodes, f.component_of.data(), f.family_off.data(), f.family_genes.data(), f.is_node.data(), f.collides.data()}, b.base,
                          c->d_gen, c->G);
        PDL_HIP(hipStreamSynchronize(c->stream));      // (c->fam may change under a later call, before the stream is waited for)
        b.base_serial = c->fam_serial;
    }
    return b.base.view(N, c->d_gen, c->G);
}

// A query's edges as the C arrays the caller gets, in the host's insertion order: n[0] of phase 1, then n[1] of phase 2.
// -> h: where src, dst, score of phase 1 (h[0..2]) and of phase 2 (h[3..5]) go
static void place_c_edges(pdl_place_result &r, const uint64_t n[2], uint8_t *h[6]) {
    pdl_place_result::CEdges &ce = r.c_edges;
    ce.drop();
    ce.n = n[0] + n[1];
    const size_t bytes = std::max<size_t>(ce.n, 1) * 4;
    ce.src = static_cast<int32_t *>(malloc(bytes)); ce.dst = static_cast<int32_t *>(malloc(bytes)); ce.score = static_cast<float *>(malloc(bytes));
    if (!ce.src || !ce.dst || !ce.score) throw std::bad_alloc();
    uint8_t *const arr[3] = {reinterpret_cast<uint8_t *>(ce.src), reinterpret_cast<uint8_t *>(ce.dst), reinterpret_cast<uint8_t *>(ce.score)};
    for (int i = 0; i < 6; i++) h[i] = arr[i % 3] + (i < 3 ? 0 : n[0] * 4);
    r.edges_phase1 = (uint32_t) n[0];
}

// pdl_place_query behind its refusals: the families of the context are valid (c->fam)
void pdl_run_place_query(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, uint32_t n, pdl_place_result &out, pdl_query_info *info) {
    hipStream_t st = c->stream;
    out = pdl_place_result{};
    const PlaceBase B = place_context_base(c);
    const pdl_query_cells run = pdl_run_query_device(c, residues, offsets, n);        // (its argument and domain refusals leave from here)
    const uint32_t N = c->N;
    const uint64_t Z = run.Z;
    if (Z >= 0x7fffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "more than 2^31 cells in the query block");
    uint64_t *d_tot = place_begin(c) + PDL_PL_EDGES_1;
    QSpans &spans = c->pb.spans;
    spans.start(st);
    spans.begin();
    uint64_t ne[2] = {0, 0};
    BbhEdges e{};
    if (Z) {                                          // P-bbh: one block, one task
        const float *cf = run.cells;
        e = bbh_edges(c, cf, reinterpret_cast<const int32_t *>(cf + 3 * run.cap), reinterpret_cast<const int32_t *>(cf + 4 * run.cap),
                      [&](const uint32_t *) { return BbhQueryBlock{c->d_gen, N, c->G}; }, run.MS, run.CM, N + n, c->G + 1, 1, n, Z, c->pb.bbh,
                      d_tot, nullptr, 1);
        spans.end();
        std::vector<uint64_t> e1, e2;
        bbh_read_counts(c, "K-place", d_tot, e, nullptr, 1, Z, 0, e1, e2);
        ne[0] = e1[1]; ne[1] = e2[1];
        spans.begin();
    }
    out.device_ms = place_run<PlaceOne>(c, B, PlaceQueries::one(N, n, ne[0], ne[1]), e.src, e.dst, true, false, spans, &out) + run.device_ms();
    // the edges themselves, straight into the caller's arrays
    uint8_t *h[6];
    place_c_edges(out, ne, h);
    bbh_copy_out(st, e, ne, h);
    if (ne[0] + ne[1]) PDL_HIP(hipStreamSynchronize(st));
    if (info) run.info_of(0, run.residues, run.kmers, run.device_ms(), info);
}

// pdl_placement_of_edges behind its argument checks: the same stages over a caller's list on a caller's base (device pointers)
void pdl_run_place_edges(pdl_ctx *c, const PlaceBase &base, uint32_t n_query, const int32_t *d_src, const int32_t *d_dst, uint64_t n_edges, pdl_place_result &out) {
    hipStream_t st = c->stream;
    out = pdl_place_result{};
    uint64_t *ctl = place_begin(c);
    QSpans &spans = c->pb.spans;
    spans.start(st);
    spans.begin();
    if (n_edges) {                                    // P-check
        const uint32_t N = base.N, NC = N + n_query;
        hipLaunchKernelGGL(k_place_check, grid256(n_edges), dim3(256), 0, st, d_src, d_dst, (uint32_t) n_edges, N, NC, ctl + PDL_PL_BAD_EDGES);
        const uint64_t bad = pdl_gate(c, spans, ctl + PDL_PL_BAD_EDGES);
        if (bad) PDL_FAIL(PDL_ERR_ARGUMENT, "K-place: %llu edges name a gene id outside [0, %u) or join two base genes (ids below %u)", (unsigned long long) bad, NC, N);
    }
    const int32_t *src[2] = {d_src, nullptr}, *dst[2] = {d_dst, nullptr};
    out.device_ms = place_run<PlaceOne>(c, base, PlaceQueries::one(base.N, n_query, n_edges, 0), src, dst, false, true, spans, &out);
}
