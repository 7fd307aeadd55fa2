// pdl_families.h — K-fam: the gene families' raw material from the network's edges where they lie (pdl_compute_families,
// pdl_families_of_edges; included at the end of pdl_bbh.hip).  What netclu_ng.py computes before it has to think — the
// connected components of the network (:58-66), and per component the test "two genes of one genome that are not adjacent"
// (get_max_collision, :75-92) — is a data-parallel graph problem; only the components that do hold a collision go on to the
// host's Girvan-Newman split (pandelos_amd/netclu.py, families_from_components).
//
// An edge is undirected, a repeated pair is one edge, a self edge makes its gene a node but is no edge (netclu.read_net).
//
//   F-check    k_fam_check      (caller's edge lists only) ids outside [0, N) counted; the host reads the count BEFORE anything
//                               below runs, so a bad id never indexes an array
//   F-cc       k_fam_union      lock-free union-find: per edge both roots by path halving, the larger root hooked under the
//                               smaller by compare-and-swap, retried; marks "is a node" per gene
//              k_fam_flatten    every gene's root (halving on the way) -> component_of
//   F-degree   k_fam_intra      same_deg[g] = distinct neighbours of g's own genome: one atomic add per end of every
//                               intra-genome edge.  K-bbh's phase-2 edges are distinct pairs (one cell per (row, column) of a
//                               genome task, row < column, and an intra-genome pair is a cell of that genome's task alone); a
//                               caller's list is compacted to (lo, hi) keys, sorted and counted at the run heads.
//   F-members  pdl_sort_pairs   (label, gene) with ascending gene ids in: members sorted by id; run heads + one scan ->
//                               family_off, the family index of every label, the node count
//   F-collide  pdl_sort_pairs   genes by genome, then stably by label: (label, genome) runs.  A run of m >= 2 genes is clean
//              k_fam_collide    exactly when every gene of it has same_deg == m - 1 (its same-genome neighbours all lie in
//                               its own run); any other gene flags its component.
//   F-out      one PinRead of the three counts, then the arrays.
//
// Why a component's label is its smallest gene id whatever the races do: parent[x] <= x always (a root is only ever hooked under
// a smaller id, halving replaces a parent by an ancestor), so a tree's root is its smallest member, and when the edges are used
// up every component is one tree.  The same invariant is what makes stale reads harmless: the per-XCD L2s are not coherent with
// each other, so a load of parent[] may return an OLDER value — but every value parent[x] ever held is an ancestor of x in the
// present forest as well.  Two finds that meet therefore prove "same tree"; a find that stops at a node which has meanwhile been
// hooked loses its compare-and-swap (the CAS executes at the memory side, coherently) and goes on from the parent the CAS
// returned.  Every step of every loop moves to a strictly smaller id, so all of them end.  parent[] is read with agent-scope
// atomic loads (sc1: served by L2, never by the CU's L1) and halved with agent-scope atomic stores.
#pragma once

#include "pdl_common.h"
#include "pdl_scan.h"
#include "pdl_sort.h"

#include <cstring>

__device__ __forceinline__ uint32_t fam_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t fam_find(uint32_t *parent, uint32_t x) {
    for (;;) {
        const uint32_t p = fam_load(parent + x);
        if (p == x) return x;
        const uint32_t gp = fam_load(parent + p);
        if (gp == p) return p;
        __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // halving: x is no root and never becomes one again
        x = gp;
    }
}

__device__ __forceinline__ void fam_union(uint32_t *parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = fam_find(parent, a); b = fam_find(parent, b);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        a = old; b = lo;                 // hi had been hooked already: go on from where it hangs
    }
}

// parent[i] = i, everything else of a run cleared; the control words of K-fam (PDL_CTL_FAM_*) with it
__global__ __launch_bounds__(256) void k_fam_init(uint32_t *parent, uint32_t *same_deg, uint8_t *is_node, uint8_t *collides, uint32_t n, uint64_t *ctl) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) { parent[i] = i; same_deg[i] = 0; is_node[i] = 0; collides[i] = 0; }
    if (i >= PDL_CTL_FAM_FIRST && i <= PDL_CTL_FAM_LAST) ctl[i] = 0;
}

__global__ __launch_bounds__(256) void k_fam_check(const int32_t *src, const int32_t *dst, uint32_t n_edges, uint32_t n, uint64_t *d_bad) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    if ((uint32_t) src[e] >= n || (uint32_t) dst[e] >= n) atomicAdd(reinterpret_cast<unsigned long long *>(d_bad), 1ull);     // (a negative id is a large unsigned one)
}

// mirrored: the list holds every pair in both directions ((r, c) then (c, r), K-bbh's phase 1), so the half with src < dst is enough
__global__ __launch_bounds__(256) void k_fam_union(const int32_t *src, const int32_t *dst, uint32_t n_edges, uint32_t mirrored, uint32_t *parent,
                                                   uint8_t *is_node) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const uint32_t a = (uint32_t) src[e], b = (uint32_t) dst[e];
    if (mirrored && a > b) return;
    is_node[a] = 1; is_node[b] = 1;
    if (a != b) fam_union(parent, a, b);
}

// component_of[i] = the root; key[i] = the sort key of F-members (the label, `n` for a gene that is no node: behind every label);
// gkey[i] = the key of F-collide's first sort
__global__ __launch_bounds__(256) void k_fam_flatten(uint32_t *parent, const uint8_t *is_node, const uint32_t *genome_of, uint32_t n, uint32_t *comp, uint32_t *key,
                                                     uint32_t *gkey) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = fam_find(parent, i);
    comp[i] = r;
    key[i] = is_node[i] ? r : n;
    gkey[i] = genome_of[i];
}

__global__ __launch_bounds__(256) void k_fam_intra(const int32_t *src, const int32_t *dst, uint32_t n_edges, const uint32_t *genome_of, uint32_t *same_deg) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const uint32_t a = (uint32_t) src[e], b = (uint32_t) dst[e];
    if (a == b || genome_of[a] != genome_of[b]) return;
    atomicAdd(same_deg + a, 1u); atomicAdd(same_deg + b, 1u);
}
// a caller's list: intra-genome edges as (lo << 32 | hi) keys, compacted ...
struct FamIntraFlag {
    const int32_t *src, *dst; const uint32_t *genome_of;
    __device__ uint32_t operator()(uint64_t e) const { const uint32_t a = (uint32_t) src[e], b = (uint32_t) dst[e]; return (uint32_t) (a != b && genome_of[a] == genome_of[b]); }
};
struct FamIntraApply {
    const int32_t *src, *dst; unsigned long long *keys;
    __device__ void operator()(uint64_t e, uint32_t f, uint32_t pre) const {
        if (!f) return;
        const uint32_t a = (uint32_t) src[e], b = (uint32_t) dst[e];
        keys[pre] = (unsigned long long) (a < b ? a : b) << 32 | (a < b ? b : a);
    }
};
// ... sorted, and counted once per run of equal keys (same_deg[0] belongs to gene id0: K-place keeps the query genes' only)
__global__ __launch_bounds__(256) void k_fam_intra_sorted(const unsigned long long *keys, const uint64_t *d_n, uint32_t *same_deg, uint32_t id0) {
    const uint64_t j = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (j >= *d_n) return;
    const unsigned long long k = keys[j];
    if (j && keys[j - 1] == k) return;
    atomicAdd(same_deg + ((uint32_t) (k >> 32) - id0), 1u); atomicAdd(same_deg + ((uint32_t) k - id0), 1u);
}

// key2[j] = label of the j-th gene in genome order (the keys of F-collide's second, stable sort)
__global__ __launch_bounds__(256) void k_fam_gather_keys(const uint32_t *genes, const uint32_t *comp, const uint8_t *is_node, uint32_t n, uint32_t *key2) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t g = genes[j];
    key2[j] = is_node[g] ? comp[g] : n;
}

// Run heads over keys sorted by label (genes that are no node carry `none` and lie behind all labels).  Without genome_of: runs
// of one label = families; off[f] = first position, index_of[label] = f, *d_nodes = positions in front of the first `none`.
// With genome_of: runs of one (label, genome); off[r] = first position, index_of[position] = r.
struct FamHeadFlag {
    const uint32_t *key, *gene, *genome_of; uint32_t none;
    __device__ uint32_t operator()(uint64_t j) const {
        const uint32_t k = key[j];
        if (k == none) return 0u;
        if (j == 0 || key[j - 1] != k) return 1u;
        return genome_of ? (uint32_t) (genome_of[gene[j - 1]] != genome_of[gene[j]]) : 0u;
    }
};
struct FamHeadApply {
    const uint32_t *key; const uint32_t *genome_of; uint32_t none, n;
    uint32_t *off, *index_of; uint64_t *d_nodes;
    __device__ void operator()(uint64_t j, uint32_t f, uint32_t pre) const {
        const uint32_t k = key[j];
        if (k == none) return;
        if (f) off[pre] = (uint32_t) j;
        if (genome_of) index_of[j] = pre + f - 1; else if (f) index_of[k] = pre;
        if (j + 1 == n || key[j + 1] == none) {           // the last node closes the list
            off[pre + f] = (uint32_t) j + 1;
            if (d_nodes) *d_nodes = j + 1;
        }
    }
};

__global__ __launch_bounds__(256) void k_fam_collide(const uint32_t *key, const uint32_t *gene, const uint32_t *run_of, const uint32_t *run_off, const uint32_t *same_deg,
                                                     const uint32_t *family_of_label, uint32_t n, uint8_t *collides) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t k = key[j];
    if (k == n) return;
    const uint32_t r = run_of[j], m = run_off[r + 1] - run_off[r];
    if (m >= 2 && same_deg[gene[j]] != m - 1) collides[family_of_label[k]] = 1;
}
__global__ __launch_bounds__(256) void k_fam_count(const uint8_t *collides, uint32_t n, const uint64_t *d_families, uint64_t *d_colliding) {
    __shared__ uint32_t s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    pdl_sync();
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f < n && f < *d_families && collides[f]) atomicAdd(&s_cnt, 1u);
    pdl_sync();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(reinterpret_cast<unsigned long long *>(d_colliding), (unsigned long long) s_cnt);
}

// One run of K-fam.  list[0] / list[1]: device edge lists (K-bbh's two phases, or a caller's list and nothing).  mirrored0: list 0
// holds every pair in both directions.  check_ids / dedupe_intra: a caller's list — ids are checked first, and the intra-genome
// edges (looked for in list 0) may repeat; otherwise they are list 1's, distinct.
void pdl_run_families(pdl_ctx *c, const int32_t *const src[2], const int32_t *const dst[2], const uint64_t n_edges[2], bool mirrored0, bool check_ids,
                      bool dedupe_intra, const uint32_t *d_gen, uint32_t N, uint32_t genome_bits, pdl_fam_result &out) {
    hipStream_t st = c->stream;
    out = pdl_fam_result{};
    out.sequences = N;
    out.family_off.assign(1, 0);
    if (N == 0) {
        if (n_edges[0] + n_edges[1]) PDL_FAIL(PDL_ERR_ARGUMENT, "K-fam: %llu edges on no gene", (unsigned long long) (n_edges[0] + n_edges[1]));
        return;
    }
    if (N >= 0x7fffffffu || n_edges[0] >= 0x7fffffffull || n_edges[1] >= 0x7fffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "K-fam: 2^31 genes or edges and more");
    pdl_ctx::FamBufs &b = c->fb;
    b.spans.start(st);
    pdl_ctl_ready(c);
    uint64_t *ctl = c->scalars.as<uint64_t>();
    const size_t n4 = (size_t) N * sizeof(uint32_t);
    b.parent.alloc(n4); b.comp.alloc(n4); b.same_deg.alloc(n4); b.is_node.alloc(N); b.collides.alloc(N);
    for (DevBuf *d : {&b.mk_a, &b.mk_b, &b.mv_a, &b.mv_b, &b.ck_a, &b.ck_b, &b.cv_a, &b.cv_b, &b.fam_of_label, &b.run_of}) d->alloc(n4);
    b.fam_off.alloc(n4 + 4); b.run_off.alloc(n4 + 4);
    uint32_t *parent = b.parent.as<uint32_t>(), *comp = b.comp.as<uint32_t>(), *same_deg = b.same_deg.as<uint32_t>();
    uint8_t *is_node = b.is_node.as<uint8_t>(), *collides = b.collides.as<uint8_t>();

    b.spans.begin();
    hipLaunchKernelGGL(k_fam_init, grid256(std::max<uint32_t>(N, PDL_CTL_FAM_LAST + 1)), dim3(256), 0, st, parent, same_deg, is_node, collides, N, ctl);
    if (check_ids && n_edges[0]) {
        hipLaunchKernelGGL(k_fam_check, grid256(n_edges[0]), dim3(256), 0, st, src[0], dst[0], (uint32_t) n_edges[0], N, ctl + PDL_CTL_FAM_BAD_IDS);
        const uint64_t bad = pdl_gate(c, b.spans, ctl + PDL_CTL_FAM_BAD_IDS);
        if (bad) PDL_FAIL(PDL_ERR_ARGUMENT, "K-fam: %llu edges name a gene id outside [0, %u)", (unsigned long long) bad, N);
    }
    // F-cc
    for (int l = 0; l < 2; l++)
        if (n_edges[l]) hipLaunchKernelGGL(k_fam_union, grid256(n_edges[l]), dim3(256), 0, st, src[l], dst[l], (uint32_t) n_edges[l], (uint32_t) (l == 0 && mirrored0), parent, is_node);
    uint32_t *mk_in = b.mk_a.as<uint32_t>(), *mk_out = b.mk_b.as<uint32_t>(), *mv_in = b.mv_a.as<uint32_t>(), *mv_out = b.mv_b.as<uint32_t>();
    uint32_t *ck_in = b.ck_a.as<uint32_t>(), *ck_out = b.ck_b.as<uint32_t>(), *cv_in = b.cv_a.as<uint32_t>(), *cv_out = b.cv_b.as<uint32_t>();
    hipLaunchKernelGGL(k_fam_flatten, grid256(N), dim3(256), 0, st, parent, is_node, d_gen, N, comp, mk_in, ck_in);
    PDL_HIP(hipGetLastError());
    // F-degree
    if (dedupe_intra) {
        const uint64_t E = n_edges[0];
        if (E) {
            b.ek_a.alloc(E * 8); b.ek_b.alloc(E * 8); b.ev_a.alloc(E * 4); b.ev_b.alloc(E * 4);
            unsigned long long *ek_in = b.ek_a.as<unsigned long long>(), *ek_out = b.ek_b.as<unsigned long long>();
            uint32_t *ev_in = b.ev_a.as<uint32_t>(), *ev_out = b.ev_b.as<uint32_t>();
            uint64_t *d_intra = ctl + PDL_CTL_FAM_INTRA;
            scan_and_apply(c, E, FamIntraFlag{src[0], dst[0], d_gen}, FamIntraApply{src[0], dst[0], ek_in}, d_intra);
            uint64_t *k_in = reinterpret_cast<uint64_t *>(ek_in), *k_out = reinterpret_cast<uint64_t *>(ek_out);
            pdl_sort_pairs<uint64_t, uint32_t>(c, k_in, k_out, ev_in, ev_out, E, 32 + bit_length64(N - 1), true, d_intra, 0, true);
            hipLaunchKernelGGL(k_fam_intra_sorted, grid256(E), dim3(256), 0, st, reinterpret_cast<const unsigned long long *>(k_out), d_intra, same_deg, 0u);
        }
    } else if (n_edges[1]) {
        hipLaunchKernelGGL(k_fam_intra, grid256(n_edges[1]), dim3(256), 0, st, src[1], dst[1], (uint32_t) n_edges[1], d_gen, same_deg);
    }
    PDL_HIP(hipGetLastError());
    // F-members: (label, gene)
    const uint32_t label_bits = bit_length64(N);                 // (labels < N, `N` itself for the genes that are no node)
    pdl_sort_pairs<uint32_t, uint32_t>(c, mk_in, mk_out, mv_in, mv_out, N, label_bits, true, nullptr, 0, true);
    uint32_t *fam_off = b.fam_off.as<uint32_t>(), *fam_of_label = b.fam_of_label.as<uint32_t>();
    scan_and_apply(c, N, FamHeadFlag{mk_out, mv_out, nullptr, N}, FamHeadApply{mk_out, nullptr, N, N, fam_off, fam_of_label, ctl + PDL_CTL_FAM_NODES},
                   ctl + PDL_CTL_FAM_FAMILIES);
    // F-collide: (label, genome) runs
    pdl_sort_pairs<uint32_t, uint32_t>(c, ck_in, ck_out, cv_in, cv_out, N, genome_bits, true, nullptr, 0, true);
    hipLaunchKernelGGL(k_fam_gather_keys, grid256(N), dim3(256), 0, st, cv_out, comp, is_node, N, ck_in);        // (ck_in is free: the sorted genes are in cv_out)
    std::swap(cv_in, cv_out);                                                                                     // in: genes by genome; out: the free half (ck_out: the genome keys, done with)
    pdl_sort_pairs<uint32_t, uint32_t>(c, ck_in, ck_out, cv_in, cv_out, N, label_bits, false, nullptr, 0, true);
    uint32_t *run_off = b.run_off.as<uint32_t>(), *run_of = b.run_of.as<uint32_t>();
    scan_and_apply(c, N, FamHeadFlag{ck_out, cv_out, d_gen, N}, FamHeadApply{ck_out, d_gen, N, N, run_off, run_of, nullptr}, ctl + PDL_CTL_FAM_RUNS);
    hipLaunchKernelGGL(k_fam_collide, grid256(N), dim3(256), 0, st, ck_out, cv_out, run_of, run_off, same_deg, fam_of_label, N, collides);
    hipLaunchKernelGGL(k_fam_count, grid256(N), dim3(256), 0, st, collides, N, ctl + PDL_CTL_FAM_FAMILIES, ctl + PDL_CTL_FAM_COLLIDING);
    PDL_HIP(hipGetLastError());
    b.spans.end();
    // F-out: the counts in one read, then the arrays
    {
        PinRead rd(c);
        const uint64_t *w = rd.add<uint64_t>(ctl + PDL_CTL_FAM_NODES, PDL_CTL_FAM_COLLIDING - PDL_CTL_FAM_NODES + 1);
        rd.sync();
        out.nodes = (uint32_t) w[0]; out.families = (uint32_t) w[PDL_CTL_FAM_FAMILIES - PDL_CTL_FAM_NODES];
        out.colliding = (uint32_t) w[PDL_CTL_FAM_COLLIDING - PDL_CTL_FAM_NODES];
    }
    if (out.nodes > N || out.families > out.nodes || out.colliding > out.families)
        PDL_FAIL(PDL_ERR_DEVICE, "K-fam: inconsistent counts (%u nodes, %u families, %u colliding of %u genes)", out.nodes, out.families, out.colliding, N);
    copy_down(st, out.component_of, comp, N); copy_down(st, out.is_node, is_node, N);
    if (out.families) { copy_down(st, out.family_off, fam_off, (size_t) out.families + 1); copy_down(st, out.family_genes, mv_out, out.nodes); copy_down(st, out.collides, collides, out.families); }
    PDL_HIP(hipStreamSynchronize(st));
    out.device_ms = b.spans.total_ms();
}
