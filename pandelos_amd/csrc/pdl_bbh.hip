// pdl_bbh.hip — K-bbh: the bidirectional-best-hit filter that the reference's Java host applies to every genome's Scores
// block (ig/infoasys/cli/pangenes/Pangenes.java:98-176), run over the cells where they already are — in HBM, right behind
// K-order — so that only the network edges cross PCIe instead of every cell and both maxima tables.
//
//   phase 1 (:98-128)   a cell (row, col) of two different genomes is a best hit in both directions when its score equals
//                       the row's best against the column's genome (max_genome_score) and the column's best against this
//                       genome (max_genome_score_col); both directions become edges.  inter_max_score[g2] = the largest
//                       such score below 1 per other genome.
//   threshold (:146-155) scoresRowThreshold[row] = min over the row's best-hit edges of inter_max_score[g2]; +inf without one
//   phase 2 (:164-175)  a cell inside one genome (row < col) is kept when it is the best of both genes inside the genome
//                       and not below the row's threshold.
// All comparisons are on the float32 values as computed (bit-identical to the reference's, see pdl_join.hip).
// Edges leave in the host's insertion order: per genome task, phase-1 edges cell by cell ((row, col) then (col, row)),
// then the phase-2 edges.
// The host side is one body for every owner of cells (the context's tasks, a query block, a chunk of queries), each over its own
// BbhBufs: bbh_edges, bbh_read_counts, bbh_copy_out.
#include "pdl_common.h"
#include "pdl_scan.h"

// Where a cell's row and column sit in the maxima tables.  BbhTasks: the genome tasks of a scored context.  pdl_place.h adds the
// one task of a query block (BbhQueryBlock), pdl_place_batch.h the queries of a chunk (BbhQueryChunk), where a gene id alone does
// not say whose it is: `part` is what the locator makes of the cell's index (nothing, for the first two).  The three kernels
// below are the filter for all.
struct BbhTasks {
    const uint32_t *taskpos_of, *task_lg, *genome_of;
    __device__ uint32_t part(uint32_t) const { return 0u; }
    __device__ uint32_t pos(uint32_t, uint32_t gene) const { return taskpos_of[gene]; }    // row of MS / thr
    __device__ uint32_t task(uint32_t, uint32_t p) const { return task_lg[p]; }            // row of CM / inter_max
    __device__ uint32_t cm_at(uint32_t) const { return 0u; }                               // where the task's CM row starts inside its N floats
    __device__ uint32_t genome(uint32_t gene) const { return genome_of[gene]; }
};
template <class L>
struct BbhArgs {
    const float *score; const int32_t *row, *col;
    L at;
    const float *MS, *CM;
    uint32_t N, G, Z;
    uint32_t *inter_max;       // [shard][G] float bits, zero-initialised
    uint32_t *thr;             // [rows] float bits, +inf-initialised
    uint8_t *kind;             // [Z] 0: no edge | 1: best hit in both directions | 2: kept intra-genome cell
};

template <class L>
__global__ __launch_bounds__(256) void k_bbh_mark(BbhArgs<L> a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.Z) return;
    const uint32_t r = (uint32_t) a.row[i], c = (uint32_t) a.col[i];
    const uint32_t w = a.at.part(i), p = a.at.pos(w, r), lg = a.at.task(w, p);
    const uint32_t g1 = a.at.genome(r), g2 = a.at.genome(c);
    const float s = a.score[i];
    const bool bbh = g1 != g2 && s == a.MS[(size_t) p * a.G + g2] && s == a.CM[(size_t) lg * a.N + a.at.cm_at(w) + c];
    a.kind[i] = bbh ? 1 : 0;
    if (bbh && s < 1.0f) atomicMax(&a.inter_max[(size_t) lg * a.G + g2], __float_as_uint(s));       // (positive floats order like their bits)
}
template <class L>
__global__ __launch_bounds__(256) void k_bbh_threshold(BbhArgs<L> a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.Z || a.kind[i] != 1) return;
    const uint32_t r = (uint32_t) a.row[i];
    const uint32_t w = a.at.part(i), p = a.at.pos(w, r), lg = a.at.task(w, p);
    atomicMin(&a.thr[p], a.inter_max[(size_t) lg * a.G + a.at.genome((uint32_t) a.col[i])]);
}
template <class L>
__global__ __launch_bounds__(256) void k_bbh_intra(BbhArgs<L> a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.Z || a.kind[i] == 1) return;
    const uint32_t r = (uint32_t) a.row[i], c = (uint32_t) a.col[i];
    const uint32_t g = a.at.genome(r);
    if (g != a.at.genome(c) || r >= c) return;
    const uint32_t w = a.at.part(i), p = a.at.pos(w, r), pc = a.at.pos(w, c);
    const float s = a.score[i];
    if (s == a.MS[(size_t) p * a.G + g] && s == a.MS[(size_t) pc * a.G + g] && s >= __uint_as_float(a.thr[p])) a.kind[i] = 2;
}

struct KindFlag {
    const uint8_t *kind; uint8_t want;
    __device__ uint32_t operator()(uint64_t i) const { return (uint32_t) (kind[i] == want); }
};
struct EdgeApply {          // phase 1 writes two edges per cell, phase 2 one; prefix[i] = cells of the kind before cell i
    const float *score; const int32_t *row, *col;
    int32_t *src, *dst; float *sc; uint32_t *prefix; uint32_t per_cell;
    __device__ void operator()(uint64_t i, uint32_t f, uint32_t pre) const {
        prefix[i] = pre;
        if (!f) return;
        const uint32_t e = pre * per_cell;
        src[e] = row[i]; dst[e] = col[i]; sc[e] = score[i];
        if (per_cell == 2) { src[e + 1] = col[i]; dst[e + 1] = row[i]; sc[e + 1] = score[i]; }
    }
};
__global__ void k_fill_u32(uint32_t *p, uint32_t n, uint32_t v) { const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) p[i] = v; }
// out[i] = pre1[at[i]], out[n + i] = pre2[at[i]]   (cells of each kind before every genome block)
__global__ void k_pick_prefixes(const uint32_t *pre1, const uint32_t *pre2, const uint32_t *at, uint32_t n, uint32_t z, uint32_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && at[i] < z) { out[i] = pre1[at[i]]; out[n + i] = pre2[at[i]]; }
}

// From cells to edges: the filter (mark, threshold, intra) over the Z cells (0 < Z < 2^31) of `tasks` tasks with `rows` rows in all —
// MS [rows][max_stride], a task's CM slice per cm_stride floats —, then the two kinds compacted in cell order into b's edge lists
// (phase 1: two edges per cell), their totals of cells to d_tot[0] / [1].  block_at [nb + 1] (host, alive until the counts have
// been read; nullptr: one block): the blocks' first cells go to the device — make_at(that copy) is the locator — and for more than
// one block the cells of each kind before each are picked.  -> the two edge lists and the picks [2][nb + 1], on the device
struct BbhEdges { int32_t *src[2], *dst[2]; float *sc[2]; uint32_t *pick; };
template <class MakeAt, class L = std::invoke_result_t<MakeAt, const uint32_t *>>
static BbhEdges bbh_edges(pdl_ctx *c, const float *score, const int32_t *row, const int32_t *col, const MakeAt &make_at, const float *MS, const float *CM,
                          uint32_t cm_stride, uint32_t max_stride, uint32_t tasks, uint32_t rows, uint64_t Z, BbhBufs &b, uint64_t *d_tot,
                          const uint32_t *block_at, uint32_t nb) {
    hipStream_t st = c->stream;
    const size_t n_max = (size_t) tasks * max_stride;
    b.kind.alloc(Z + 16);
    b.tab.alloc((n_max + rows + 2 * (Z + 1) + 3 * ((size_t) nb + 1)) * sizeof(uint32_t));
    b.e_src.alloc(3 * Z * sizeof(int32_t)); b.e_dst.alloc(3 * Z * sizeof(int32_t)); b.e_score.alloc(3 * Z * sizeof(float));
    uint32_t *inter_max = b.tab.as<uint32_t>(), *thr = inter_max + n_max, *pre1 = thr + rows, *pre2 = pre1 + (Z + 1), *d_at = pre2 + (Z + 1);
    if (block_at) PDL_HIP(hipMemcpyAsync(d_at, block_at, ((size_t) nb + 1) * 4, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemsetAsync(inter_max, 0, n_max * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_fill_u32, grid256(rows), dim3(256), 0, st, thr, rows, 0x7f800000u);
    const BbhArgs<L> a{score, row, col, make_at((const uint32_t *) d_at), MS, CM, cm_stride, max_stride, (uint32_t) Z, inter_max, thr, b.kind.as<uint8_t>()};
    hipLaunchKernelGGL(k_bbh_mark<L>, grid256(Z), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_bbh_threshold<L>, grid256(Z), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_bbh_intra<L>, grid256(Z), dim3(256), 0, st, a);
    PDL_HIP(hipGetLastError());
    int32_t *src = b.e_src.as<int32_t>(), *dst = b.e_dst.as<int32_t>(); float *sc = b.e_score.as<float>();
    BbhEdges e{{src, src + 2 * Z}, {dst, dst + 2 * Z}, {sc, sc + 2 * Z}, nullptr};
    scan_and_apply(c, Z, KindFlag{a.kind, 1}, EdgeApply{score, row, col, e.src[0], e.dst[0], e.sc[0], pre1, 2}, d_tot);
    scan_and_apply(c, Z, KindFlag{a.kind, 2}, EdgeApply{score, row, col, e.src[1], e.dst[1], e.sc[1], pre2, 1}, d_tot + 1);
    if (nb > 1) {           // the prefixes at every block's first cell (the totals close the lists)
        e.pick = d_at + (nb + 1);
        hipLaunchKernelGGL(k_pick_prefixes, grid256((uint64_t) nb + 1), dim3(256), 0, st, pre1, pre2, d_at, nb + 1, (uint32_t) Z, e.pick);
        PDL_HIP(hipGetLastError());
    }
    return e;
}
// The counts of that run in one read, totals and picks -> every block's first phase-1 and first phase-2 edge (bbh_cut_blocks)
static void bbh_read_counts(pdl_ctx *c, const char *who, const uint64_t *d_tot, const BbhEdges &e, const uint32_t *block_at, uint32_t nb, uint64_t Z, uint32_t block0,
                            std::vector<uint64_t> &e1, std::vector<uint64_t> &e2) {
    PinRead rd(c);
    const uint64_t *pt = rd.add<uint64_t>(d_tot, 2);
    const uint32_t *pp = e.pick ? rd.add<uint32_t>(e.pick, 2 * ((size_t) nb + 1)) : nullptr;
    rd.sync();
    bbh_cut_blocks(who, pt[0], pt[1], pp, block_at, nb, Z, block0, e1, e2);
}
// The n[0] + n[1] edges come down (queued): src, dst, score of phase 1 to h[0..2], of phase 2 to h[3..5] — which, given m, are
// first laid out in that one pinned piece: src1 | dst1 | sc1 | src2 | dst2 | sc2
static void bbh_copy_out(hipStream_t st, const BbhEdges &e, const uint64_t n[2], uint8_t *h[6], uint8_t *m = nullptr) {
    const void *d[6] = {e.src[0], e.dst[0], e.sc[0], e.src[1], e.dst[1], e.sc[1]};
    for (int i = 0; i < 6; i++) {
        if (m) h[i] = m + (i < 3 ? i * n[0] : 3 * n[0] + (i - 3) * n[1]) * 4;
        if (n[i / 3]) PDL_HIP(hipMemcpyAsync(h[i], d[i], n[i / 3] * 4, hipMemcpyDeviceToHost, st));
    }
}

// Runs the filter for every genome task of the context; leaves the edges on the host (pinned), per genome
// [phase-1 edges | phase-2 edges].
void pdl_run_bbh_all(pdl_ctx *c) {
    hipStream_t st = c->stream;
    const uint32_t S = (uint32_t) c->shard.size(), n_rows = c->n_task_rows;
    const uint64_t Z = c->h_cell_off.empty() ? 0 : c->h_cell_off.back();
    c->h_edge1.assign((size_t) S + 1, 0); c->h_edge_off.assign((size_t) S + 1, 0);
    c->edges_valid = true;
    c->fam_valid = false;              // (K-fam's answer was for the edges before these)
    if (Z == 0 || n_rows == 0) { c->n_edges = 0; return; }
    if (Z >= 0x7fffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "more than 2^31 cells on one device");
    const std::vector<uint32_t> at(c->h_cell_off.begin(), c->h_cell_off.end());       // [S + 1] every genome block's first cell
    uint64_t *d_tot = c->scalars.as<uint64_t>() + PDL_CTL_EDGES_1;
    const BbhEdges e = bbh_edges(c, c->c_score.as<float>(), c->c_row.as<int32_t>(), c->c_col.as<int32_t>(),
                                 [&](const uint32_t *) { return BbhTasks{c->taskpos_of.as<uint32_t>(), c->task_lg.as<uint32_t>(), c->d_gen}; },
                                 c->MS.as<float>(), c->CM.as<float>(), c->N, c->G, S, n_rows, Z, c->bbh, d_tot, at.data(), S);
    std::vector<uint64_t> e1, e2;                      // phase-1 edge offsets, phase-2 edge offsets
    bbh_read_counts(c, "K-bbh", d_tot, e, at.data(), S, Z, 0, e1, e2);
    const uint64_t n[2] = {e1[S], e2[S]};
    uint8_t *h[6];
    c->n_edges = n[0] + n[1];
    c->edge_mirror.alloc((size_t) c->n_edges * 12 + 64);
    bbh_copy_out(st, e, n, h, c->edge_mirror.p);
    PDL_HIP(hipStreamSynchronize(st));
    c->n_edges1 = n[0]; c->h_edge1.swap(e1); c->h_edge_off.swap(e2);
}

#include "pdl_families.h"        // K-fam: components, families and collision flags from these edges (pdl_compute_families)

// K-fam over the edges K-bbh left in e_src / e_dst: phase 1 at the front (every pair in both directions), phase 2 behind the
// room of 2 Z phase-1 edges.
void pdl_run_families_of_context(pdl_ctx *c) {
    const uint64_t Z = c->h_cell_off.empty() ? 0 : c->h_cell_off.back();
    const uint64_t n1 = c->n_edges ? c->n_edges1 : 0, n2 = c->n_edges - n1;          // (a context without a cell has no edge list at all)
    const int32_t *src[2] = {c->bbh.e_src.as<int32_t>(), c->bbh.e_src.as<int32_t>() + 2 * Z}, *dst[2] = {c->bbh.e_dst.as<int32_t>(), c->bbh.e_dst.as<int32_t>() + 2 * Z};
    const uint64_t n[2] = {n1, n2};
    pdl_run_families(c, src, dst, n, true, false, false, c->d_gen, c->N, bit_length64(c->G ? c->G - 1 : 0), c->fam);
    c->fam_valid = true;
    c->fam_serial++;                   // (K-place's device copy of c->fam is of an earlier run)
}

#include "pdl_place.h"           // K-place: a query's edges and their placement on these families (pdl_place_query)
#include "pdl_place_batch.h"     // ... for a batch of queries (pdl_place_batch)
#include "pdl_split.h"           // K-split: Girvan-Newman's first level on the components K-fam flagged (pdl_split_first_level)
#include "pdl_profile.h"         // the pan-genome profile of a labelling and pan / core curves over genome orders (pdl_family_profile, pdl_pan_curves)
#include "pdl_matrix.h"          // genome-by-genome shared-family matrices of a profile (pdl_genome_matrix)
