// pdl_place.h — K-place: a new genome's genes placed into the gene families that are already built (pdl_place_query,
// pdl_placement_of_edges; included from pdl_bbh.hip behind pdl_families.h).  The query's Scores block (K-query, pdl_query.h) is
// filtered where it lies — K-bbh's three kernels over the one task of the block — and the edges are hung onto the base network's
// components without clustering the base again: the union-find of K-fam starts from the base's labels.
//
// Ids are union ids: base genes 0..N-1, query genes N..N+n-1 (genome G).  Every edge has a query end; a base-base edge is refused.
//
//   P-bbh      k_bbh_mark/_threshold/_intra (pdl_bbh.hip) with BbhQueryBlock: row p = gene - N, one task, genome G for ids >= N;
//              the two kinds compacted in cell order (KindFlag / EdgeApply): phase 1 ((row, col) then (col, row)), phase 2
//   P-check    k_place_check    (a caller's list only) ids outside [0, N + n) and base-base edges counted; read BEFORE anything below
//   P-cc       parent[0..N) = the base's component_of (one device copy: the only O(N) step), parent[N..N+n) = identity: parent[x] <= x
//              holds from the start, so fam_union / fam_find (pdl_families.h) over the query's edges leave every tree's root its
//              smallest member.  k_place_union marks the query genes that are a node; k_place_roots: family_of and the sort keys
//   P-degree   same_deg of the query genes from the query-query edges: phase 2's distinct pairs, or a caller's list compacted to
//              (lo, hi) keys, sorted and counted at the run heads (k_fam_intra_sorted)
//   P-groups   pdl_sort_pairs (root, query gene), run heads + scan (FamHeadFlag / FamHeadApply): groups in label order, their
//              query members ascending, the group index of every label
//   P-base     edges with a base end -> (group, base label) keys, compacted, sorted, run heads: every group's fused base components;
//              a component that collides in the base flags its group (a lookup)
//   P-bridge   groups of two or more base components: their members gathered (a gene that was no node is its own), keyed by
//              (group, genome), sorted; a run with genes of two components flags the group — such genes cannot be adjacent, every
//              new edge has a query end
//   P-clique   a group's m >= 2 query genes are clean exactly when each has same_deg == m - 1 (as F-collide)
//   P-out      one PinRead of the counts (the member total sizes P-bridge), then the arrays
//
// Work: the query's edges plus the members of bridged components; of the work nothing but the parent copy is proportional to N.
// Memory is: parent and grp_of_label (indexed by label, touched at the groups' labels only) hold N + n words each.
// The kernels take the id origin N and the edge lists as arguments and keep no state between launches: pdl_place_batch.h runs
// them over every query's stretch of a chunk's edges.
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

__global__ __launch_bounds__(256) void k_place_init(uint32_t *parent_q, uint32_t *same_deg, uint8_t *is_node, uint8_t *gcol, uint32_t N, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) { parent_q[i] = N + i; same_deg[i] = 0; is_node[i] = 0; gcol[i] = 0; }
}
__global__ __launch_bounds__(256) void k_place_check(const int32_t *src, const int32_t *dst, uint32_t n_edges, uint32_t N, uint32_t NC, uint64_t *d_bad) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const uint32_t a = (uint32_t) src[e], b = (uint32_t) dst[e];                 // (a negative id is a large unsigned one)
    if (a >= NC || b >= NC || (a < N && b < N)) atomicAdd(reinterpret_cast<unsigned long long *>(d_bad), 1ull);
}
// as k_fam_union; only the query genes' node flags are kept (is_node[0] belongs to gene N)
__global__ __launch_bounds__(256) void k_place_union(const int32_t *src, const int32_t *dst, uint32_t n_edges, uint32_t mirrored, uint32_t N, uint32_t *parent,
                                                     uint8_t *is_node) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const uint32_t a = (uint32_t) src[e], b = (uint32_t) dst[e];
    if (mirrored && a > b) return;
    if (a >= N) is_node[a - N] = 1;
    if (b >= N) is_node[b - N] = 1;
    if (a != b) fam_union(parent, a, b);
}
// phase 2: distinct query-query pairs
__global__ __launch_bounds__(256) void k_place_intra(const int32_t *src, const int32_t *dst, uint32_t n_edges, uint32_t N, uint32_t *same_deg) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const uint32_t a = (uint32_t) src[e], b = (uint32_t) dst[e];
    if (a == b || a < N || b < N) return;
    atomicAdd(same_deg + (a - N), 1u); atomicAdd(same_deg + (b - N), 1u);
}
struct PlaceIntraFlag {
    const int32_t *src, *dst; uint32_t N;
    __device__ uint32_t operator()(uint64_t e) const { const uint32_t a = (uint32_t) src[e], b = (uint32_t) dst[e]; return (uint32_t) (a != b && a >= N && b >= N); }
};
// family_of[i] = the root of query gene N + i (its own id when it is no node); key[i] = the sort key of P-groups (`none` behind all)
__global__ __launch_bounds__(256) void k_place_roots(uint32_t *parent, const uint8_t *is_node, uint32_t N, uint32_t n, uint32_t *family_of, uint32_t *key) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = is_node[i] ? fam_find(parent, N + i) : N + i;
    family_of[i] = r;
    key[i] = is_node[i] ? r : N + n;
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
struct PlaceBaseApply {
    const int32_t *src, *dst; uint32_t N, label_bits;
    const uint32_t *family_of, *grp_of_label, *base_comp; unsigned long long *keys;
    __device__ void operator()(uint64_t e, uint32_t f, uint32_t pre) const {
        if (!f) return;
        const uint32_t a = (uint32_t) src[e], b = (uint32_t) dst[e];
        const uint32_t q = a < N ? b : a, g = a < N ? a : b;
        keys[pre] = (unsigned long long) grp_of_label[family_of[q - N]] << label_bits | base_comp[g];
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
    if (!c->scalars.p) c->scalars.alloc((PDL_CTL_LAST + 1) * sizeof(uint64_t));      // (a context that has built nothing yet: the sort's word is all it needs)
    c->pb.ctl.alloc(PDL_PL_WORDS * sizeof(uint64_t));
    PDL_HIP(hipMemsetAsync(c->pb.ctl.p, 0, PDL_PL_WORDS * sizeof(uint64_t), c->stream));
    return c->pb.ctl.as<uint64_t>();
}

// One placement.  list[0] / list[1]: device edge lists in union ids (the query block's two phases, or a caller's list and nothing).
// mirrored0: list 0 holds every pair in both directions.  caller: query-query edges (looked for in list 0) may repeat; otherwise
// they are list 1's, distinct.  check_ids: a caller's ids are checked first (a batch has checked all its lists at once).
// `spans` has a stretch open on entry and none on return.
// place_run_batch (pdl_place_batch.h) is its twin over the queries of a chunk, stage for stage: a change to one belongs into the other.
static void place_run(pdl_ctx *c, const PlaceBase &B, uint32_t n, const int32_t *const src[2], const int32_t *const dst[2], const uint64_t n_edges[2],
                      bool mirrored0, bool caller, bool check_ids, QSpans &spans, pdl_place_result &out) {
    hipStream_t st = c->stream;
    pdl_ctx::PlaceBufs &b = c->pb;
    const uint32_t N = B.N;
    if ((uint64_t) N + n >= 0x7fffffffull || n_edges[0] >= 0x7fffffffull || n_edges[1] >= 0x7fffffffull)
        PDL_FAIL(PDL_ERR_UNSUPPORTED, "K-place: 2^31 genes or edges and more");
    const uint32_t NC = N + n;
    uint64_t *ctl = b.ctl.as<uint64_t>();
    const size_t n4 = (size_t) n * 4;
    b.parent.alloc((size_t) NC * 4); b.grp_of_label.alloc((size_t) NC * 4);
    b.is_node.alloc(n); b.gcol.alloc(n); b.same_deg.alloc(n4); b.family_of.alloc(n4); b.gq_off.alloc(n4 + 4); b.gb_off.alloc(n4 + 4);
    for (DevBuf *d : {&b.mk_a, &b.mk_b, &b.mv_a, &b.mv_b}) d->alloc(n4);
    uint32_t *parent = b.parent.as<uint32_t>(), *same_deg = b.same_deg.as<uint32_t>(), *family_of = b.family_of.as<uint32_t>();
    uint32_t *grp_of_label = b.grp_of_label.as<uint32_t>(), *gq_off = b.gq_off.as<uint32_t>(), *gb_off = b.gb_off.as<uint32_t>();
    uint8_t *is_node = b.is_node.as<uint8_t>(), *gcol = b.gcol.as<uint8_t>();

    if (check_ids && n_edges[0]) {                    // P-check
        hipLaunchKernelGGL(k_place_check, fam_grid(n_edges[0]), dim3(256), 0, st, src[0], dst[0], (uint32_t) n_edges[0], N, NC, ctl + PDL_PL_BAD_EDGES);
        PDL_HIP(hipGetLastError());
        spans.end();
        PinRead rd(c);
        const uint64_t *bad = rd.add<uint64_t>(ctl + PDL_PL_BAD_EDGES, 1);
        rd.sync();
        if (*bad) PDL_FAIL(PDL_ERR_ARGUMENT, "K-place: %llu edges name a gene id outside [0, %u) or join two base genes (ids below %u)", (unsigned long long) *bad, NC, N);
        spans.begin();
    }
    // P-cc
    if (N) PDL_HIP(hipMemcpyAsync(parent, B.comp, (size_t) N * 4, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_place_init, fam_grid(n), dim3(256), 0, st, parent + N, same_deg, is_node, gcol, N, n);
    for (int l = 0; l < 2; l++)
        if (n_edges[l]) hipLaunchKernelGGL(k_place_union, fam_grid(n_edges[l]), dim3(256), 0, st, src[l], dst[l], (uint32_t) n_edges[l], (uint32_t) (l == 0 && mirrored0), N, parent, is_node);
    uint32_t *mk_in = b.mk_a.as<uint32_t>(), *mk_out = b.mk_b.as<uint32_t>(), *mv_in = b.mv_a.as<uint32_t>(), *mv_out = b.mv_b.as<uint32_t>();
    hipLaunchKernelGGL(k_place_roots, fam_grid(n), dim3(256), 0, st, parent, is_node, N, n, family_of, mk_in);
    PDL_HIP(hipGetLastError());
    // P-degree
    if (caller) {
        const uint64_t E = n_edges[0];
        if (E) {
            b.ek_a.alloc(E * 8); b.ek_b.alloc(E * 8); b.ev_a.alloc(E * 4); b.ev_b.alloc(E * 4);
            unsigned long long *ek_in = b.ek_a.as<unsigned long long>();
            uint32_t *ev_in = b.ev_a.as<uint32_t>(), *ev_out = b.ev_b.as<uint32_t>();
            uint64_t *d_intra = ctl + PDL_PL_INTRA;
            scan_and_apply(c, E, PlaceIntraFlag{src[0], dst[0], N}, FamIntraApply{src[0], dst[0], ek_in}, d_intra);
            uint64_t *k_in = reinterpret_cast<uint64_t *>(ek_in), *k_out = b.ek_b.as<uint64_t>();
            pdl_sort_pairs<uint64_t, uint32_t>(c, k_in, k_out, ev_in, ev_out, E, 32 + bit_length64(NC - 1), true, d_intra, 0, true);
            hipLaunchKernelGGL(k_fam_intra_sorted, fam_grid(E), dim3(256), 0, st, reinterpret_cast<const unsigned long long *>(k_out), d_intra, same_deg, N);
        }
    } else if (n_edges[1]) {
        hipLaunchKernelGGL(k_place_intra, fam_grid(n_edges[1]), dim3(256), 0, st, src[1], dst[1], (uint32_t) n_edges[1], N, same_deg);
    }
    PDL_HIP(hipGetLastError());
    // P-groups: (root, query gene), query genes ascending in
    pdl_sort_pairs<uint32_t, uint32_t>(c, mk_in, mk_out, mv_in, mv_out, n, bit_length64(NC), true, nullptr, 0, true);
    scan_and_apply(c, n, FamHeadFlag{mk_out, mv_out, nullptr, NC}, FamHeadApply{mk_out, nullptr, NC, n, gq_off, grp_of_label, ctl + PDL_PL_NODES}, ctl + PDL_PL_GROUPS);
    // P-base
    const uint64_t E0 = n_edges[0];
    const uint32_t label_bits = std::max<uint32_t>(1, bit_length64(N ? N - 1 : 0)), group_bits = std::max<uint32_t>(1, bit_length64(n));
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
                       PlaceBaseApply{src[0], dst[0], N, label_bits, family_of, grp_of_label, B.comp, reinterpret_cast<unsigned long long *>(k_in)}, d_base);
        pdl_sort_pairs<uint64_t, uint32_t>(c, k_in, k_out, v_in, v_out, E0, label_bits + group_bits, true, d_base, 0, true);
        const unsigned long long *sorted = reinterpret_cast<const unsigned long long *>(k_out);
        scan_and_apply(c, E0, PlaceUniqFlag{sorted}, PlaceUniqApply{sorted, uniq, group_base, gcol, B, label_bits}, d_pairs, nullptr, d_base);
        hipLaunchKernelGGL(k_place_base_off, fam_grid((uint64_t) n + 1), dim3(256), 0, st, uniq, d_pairs, ctl + PDL_PL_GROUPS, n, label_bits, gb_off);
        scan_and_apply(c, E0, PlaceMemberFlag{uniq, gb_off, B, label_bits}, PlaceMemberApply{mpre}, ctl + PDL_PL_MEMBERS, nullptr, d_pairs);
    }
    // P-clique
    hipLaunchKernelGGL(k_place_clique, fam_grid(n), dim3(256), 0, st, mk_out, mv_out, grp_of_label, gq_off, same_deg, ctl + PDL_PL_NODES, n, gcol);
    PDL_HIP(hipGetLastError());
    spans.end();
    // P-out: the counts in one read ...
    uint64_t nodes, groups, pairs, members;
    {
        PinRead rd(c);
        const uint64_t *w = rd.add<uint64_t>(ctl + PDL_PL_NODES, PDL_PL_MEMBERS - PDL_PL_NODES + 1);
        rd.sync();
        nodes = w[0]; groups = w[PDL_PL_GROUPS - PDL_PL_NODES]; pairs = w[PDL_PL_BASE_PAIRS - PDL_PL_NODES]; members = w[PDL_PL_MEMBERS - PDL_PL_NODES];
    }
    if (nodes > n || groups > nodes || pairs > E0 || (groups == 0 && pairs) || members >= 0x7fffffffull)
        PDL_FAIL(PDL_ERR_DEVICE, "K-place: inconsistent counts (%llu nodes, %llu groups, %llu base pairs, %llu members of %u query genes, %llu edges)",
                 (unsigned long long) nodes, (unsigned long long) groups, (unsigned long long) pairs, (unsigned long long) members, n, (unsigned long long) E0);
    // ... P-bridge, sized by the member total ...
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
    // ... then the arrays
    out.sequences = N; out.n_query = n; out.genomes = B.G; out.groups = (uint32_t) groups;
    out.family_of.resize(n); out.is_node.resize(n);
    out.group_query_off.assign(groups + 1, 0); out.group_base_off.assign(groups + 1, 0);
    out.group_query.resize(nodes); out.group_base.resize(pairs); out.group_collides.resize(groups); out.group_label.resize(groups);
    PDL_HIP(hipMemcpyAsync(out.family_of.data(), family_of, n4, hipMemcpyDeviceToHost, st));
    PDL_HIP(hipMemcpyAsync(out.is_node.data(), is_node, n, hipMemcpyDeviceToHost, st));
    if (groups) {
        PDL_HIP(hipMemcpyAsync(out.group_query_off.data(), gq_off, (groups + 1) * 4, hipMemcpyDeviceToHost, st));
        PDL_HIP(hipMemcpyAsync(out.group_query.data(), mv_out, nodes * 4, hipMemcpyDeviceToHost, st));
        PDL_HIP(hipMemcpyAsync(out.group_collides.data(), gcol, groups, hipMemcpyDeviceToHost, st));
        if (E0) PDL_HIP(hipMemcpyAsync(out.group_base_off.data(), gb_off, (groups + 1) * 4, hipMemcpyDeviceToHost, st));
        if (pairs) PDL_HIP(hipMemcpyAsync(out.group_base.data(), group_base, pairs * 4, hipMemcpyDeviceToHost, st));
    }
    PDL_HIP(hipStreamSynchronize(st));
    if (groups && (out.group_query_off[0] != 0 || out.group_query_off[groups] != nodes || out.group_base_off[groups] != pairs))
        PDL_FAIL(PDL_ERR_DEVICE, "K-place: inconsistent group offsets");
    out.unplaced = n - (uint32_t) nodes;
    for (uint64_t g = 0; g < groups; g++) {
        const uint32_t q0 = out.group_query_off[g], nb = out.group_base_off[g + 1] - out.group_base_off[g];
        if (q0 >= nodes || out.group_query[q0] >= n) PDL_FAIL(PDL_ERR_DEVICE, "K-place: inconsistent group members");
        out.group_label[g] = out.family_of[out.group_query[q0]];
        (nb == 0 ? out.novel : nb == 1 ? out.joined : out.bridging)++;
        out.colliding += out.group_collides[g] ? 1u : 0u;
    }
    for (uint32_t &q : out.group_query) q += N;       // (the sort carried the query genes' positions)
    out.device_ms = spans.total_ms();
}

// the context's own families on the device: uploaded once per run of K-fam (c->fam is its answer on the host)
static PlaceBase place_context_base(pdl_ctx *c) {
    pdl_ctx::PlaceBufs &b = c->pb;
    const pdl_fam_result &f = c->fam;
    const uint32_t N = c->N;
    if (f.sequences != N || f.component_of.size() != N) PDL_FAIL(PDL_ERR_STATE, "K-place: the context's families are not those of its %u genes", N);
    if (b.base_serial != c->fam_serial) {
        hipStream_t st = c->stream;
        b.base_serial = 0;
        std::vector<uint32_t> of_label(N, 0);
        for (uint32_t i = 0; i < f.families; i++) of_label[f.family_genes[f.family_off[i]]] = i;
        b.base_comp.alloc((size_t) N * 4); b.base_is_node.alloc(N); b.base_fam_of_label.alloc((size_t) N * 4);
        b.base_fam_off.alloc(((size_t) f.families + 1) * 4); b.base_fam_genes.alloc((size_t) f.nodes * 4); b.base_collides.alloc(f.families);
        PDL_HIP(hipMemcpyAsync(b.base_comp.p, f.component_of.data(), (size_t) N * 4, hipMemcpyHostToDevice, st));
        PDL_HIP(hipMemcpyAsync(b.base_is_node.p, f.is_node.data(), N, hipMemcpyHostToDevice, st));
        PDL_HIP(hipMemcpyAsync(b.base_fam_of_label.p, of_label.data(), (size_t) N * 4, hipMemcpyHostToDevice, st));
        PDL_HIP(hipMemcpyAsync(b.base_fam_off.p, f.family_off.data(), ((size_t) f.families + 1) * 4, hipMemcpyHostToDevice, st));
        if (f.nodes) PDL_HIP(hipMemcpyAsync(b.base_fam_genes.p, f.family_genes.data(), (size_t) f.nodes * 4, hipMemcpyHostToDevice, st));
        if (f.families) PDL_HIP(hipMemcpyAsync(b.base_collides.p, f.collides.data(), f.families, hipMemcpyHostToDevice, st));
        PDL_HIP(hipStreamSynchronize(st));
        b.base_serial = c->fam_serial;
    }
    PlaceBase B;
    B.comp = b.base_comp.as<uint32_t>(); B.is_node = b.base_is_node.as<uint8_t>(); B.collides = b.base_collides.as<uint8_t>();
    B.fam_off = b.base_fam_off.as<uint32_t>(); B.fam_genes = b.base_fam_genes.as<uint32_t>(); B.fam_of_label = b.base_fam_of_label.as<uint32_t>();
    B.genome_of = c->d_gen; B.N = N; B.G = c->G;
    return B;
}

// pdl_place_query behind its refusals: the families of the context are valid (c->fam)
void pdl_run_place_query(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, uint32_t n, pdl_place_result &out, pdl_query_info *info) {
    hipStream_t st = c->stream;
    pdl_ctx::PlaceBufs &b = c->pb;
    out = pdl_place_result{};
    const PlaceBase B = place_context_base(c);
    const pdl_query_run run = pdl_run_query_device(c, residues, offsets, n);          // (its argument and domain refusals leave from here)
    const uint32_t N = c->N, G1 = c->G + 1;
    const uint64_t Z = run.Z;
    if (Z >= 0x7fffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "more than 2^31 cells in the query block");
    uint64_t *ctl = place_begin(c);
    QSpans &spans = b.spans;
    spans.start(st);
    spans.begin();
    // P-bbh
    uint64_t n1 = 0, n2 = 0;
    int32_t *src1 = nullptr, *dst1 = nullptr, *src2 = nullptr, *dst2 = nullptr;
    float *sc1 = nullptr, *sc2 = nullptr;
    if (Z) {
        b.kind.alloc(Z + 16);
        b.tab.alloc(((size_t) G1 + n + 2 * (Z + 1)) * sizeof(uint32_t));
        uint32_t *inter_max = b.tab.as<uint32_t>(), *thr = inter_max + G1, *pre1 = thr + n, *pre2 = pre1 + (Z + 1);
        PDL_HIP(hipMemsetAsync(inter_max, 0, (size_t) G1 * sizeof(uint32_t), st));
        hipLaunchKernelGGL(k_fill_u32, dim3((n + 255) / 256), dim3(256), 0, st, thr, n, 0x7f800000u);
        const float *cf = c->qb.cells.as<float>();
        BbhArgs<BbhQueryBlock> a{};
        a.score = cf; a.row = reinterpret_cast<const int32_t *>(cf + 3 * run.cap); a.col = reinterpret_cast<const int32_t *>(cf + 4 * run.cap);
        a.at = BbhQueryBlock{c->d_gen, N, c->G};
        a.MS = c->qb.MS.as<float>(); a.CM = c->qb.CM.as<float>(); a.N = N + n; a.G = G1; a.Z = (uint32_t) Z;
        a.inter_max = inter_max; a.thr = thr; a.kind = b.kind.as<uint8_t>();
        bbh_filter(st, a);
        b.e_src.alloc(3 * Z * sizeof(int32_t)); b.e_dst.alloc(3 * Z * sizeof(int32_t)); b.e_score.alloc(3 * Z * sizeof(float));
        src1 = b.e_src.as<int32_t>(); dst1 = b.e_dst.as<int32_t>(); sc1 = b.e_score.as<float>();
        src2 = src1 + 2 * Z; dst2 = dst1 + 2 * Z; sc2 = sc1 + 2 * Z;
        scan_and_apply(c, Z, KindFlag{a.kind, 1}, EdgeApply{a.score, a.row, a.col, src1, dst1, sc1, pre1, 2}, ctl + PDL_PL_EDGES_1);
        scan_and_apply(c, Z, KindFlag{a.kind, 2}, EdgeApply{a.score, a.row, a.col, src2, dst2, sc2, pre2, 1}, ctl + PDL_PL_EDGES_2);
        spans.end();
        PinRead rd(c);
        const uint64_t *pt = rd.add<uint64_t>(ctl + PDL_PL_EDGES_1, PDL_PL_EDGES_2 - PDL_PL_EDGES_1 + 1);
        rd.sync();
        n1 = 2 * pt[0]; n2 = pt[PDL_PL_EDGES_2 - PDL_PL_EDGES_1];
        if (n1 > 2 * Z || n2 > Z) PDL_FAIL(PDL_ERR_DEVICE, "K-place: %llu + %llu edges of %llu cells", (unsigned long long) n1, (unsigned long long) n2, (unsigned long long) Z);
        spans.begin();
    }
    const int32_t *src[2] = {src1, src2}, *dst[2] = {dst1, dst2};
    const uint64_t ne[2] = {n1, n2};
    place_run(c, B, n, src, dst, ne, true, false, false, spans, out);
    // the edges themselves, in the host's insertion order: phase 1, then phase 2
    out.src.resize(n1 + n2); out.dst.resize(n1 + n2); out.score.resize(n1 + n2);
    if (n1) {
        PDL_HIP(hipMemcpyAsync(out.src.data(), src1, n1 * 4, hipMemcpyDeviceToHost, st));
        PDL_HIP(hipMemcpyAsync(out.dst.data(), dst1, n1 * 4, hipMemcpyDeviceToHost, st));
        PDL_HIP(hipMemcpyAsync(out.score.data(), sc1, n1 * 4, hipMemcpyDeviceToHost, st));
    }
    if (n2) {
        PDL_HIP(hipMemcpyAsync(out.src.data() + n1, src2, n2 * 4, hipMemcpyDeviceToHost, st));
        PDL_HIP(hipMemcpyAsync(out.dst.data() + n1, dst2, n2 * 4, hipMemcpyDeviceToHost, st));
        PDL_HIP(hipMemcpyAsync(out.score.data() + n1, sc2, n2 * 4, hipMemcpyDeviceToHost, st));
    }
    if (n1 + n2) PDL_HIP(hipStreamSynchronize(st));
    out.edges_phase1 = (uint32_t) n1;
    out.device_ms += c->qb.spans.total_ms();
    if (info) {
        memset(info, 0, sizeof(*info));
        info->residues = run.residues; info->kmer_occurrences = run.kmers; info->records = run.records; info->matched_records = run.matched;
        info->genome_cost = run.cost; info->device_ms = c->qb.spans.total_ms();
    }
}

// pdl_placement_of_edges behind its argument checks: the same kernels over a caller's list on a caller's base (device pointers)
void pdl_run_place_edges(pdl_ctx *c, const PlaceBase &base, uint32_t n_query, const int32_t *d_src, const int32_t *d_dst, uint64_t n_edges, pdl_place_result &out) {
    out = pdl_place_result{};
    (void) place_begin(c);
    QSpans &spans = c->pb.spans;
    spans.start(c->stream);
    spans.begin();
    const int32_t *src[2] = {d_src, nullptr}, *dst[2] = {d_dst, nullptr};
    const uint64_t ne[2] = {n_edges, 0};
    place_run(c, base, n_query, src, dst, ne, false, true, true, spans, out);
}
