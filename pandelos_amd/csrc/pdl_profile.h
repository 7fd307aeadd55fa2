// pdl_profile.h — the pan-genome profile of a family labelling (pdl_family_profile) and pan / core accumulation curves over
// genome orders (pdl_pan_curves); included at the end of pdl_bbh.hip.  What example/quality.py of the reference counts over a
// .clus — family sizes, genome spreads, the per-genome spread table — is three histograms over the (label, genome) runs of the
// genes; the curve over many genome orders is the part with weight: orders x (family, genome) incidences of integer work.
//
//   P-check    k_prof_check       labels >= N and genome ids >= G counted; the host reads the count BEFORE anything below runs
//   P-keys     k_prof_keys        key = label << bits(G) | genome; the genomes' gene counts
//              pdl_sort_pairs     the keys in ascending order (the values, gene ids, are carried and not read)
//   P-runs     scan_and_apply     heads of the (label, genome) runs -> the incidences: where each starts, its genome, its label
//              scan_and_apply     heads of the label runs -> the families: where each starts, its label, its first incidence
//   P-hist     k_prof_families    size, spread, their histograms, the largest size, the single-copy core
//              k_prof_incidences  copies, the per-genome spread table, the genomes' genes by class of family
//   P-out      one PinRead of the counts, then the arrays.
//
//   C-check    k_pan_check        per order: ids >= G or named twice, counted; the first failing order by an atomic minimum;
//                                 read by the host BEFORE an order indexes anything
//   C-bits     k_pan_bits         presence bit matrix F x ceil(G / 64) words from the CSR, a wave per family
//   C-hist     k_pan_curves       one workgroup = one order and a tile of PAN_TILE families.  LDS: the order, its inverse, two
//                                 histograms of G + 1 bins.  Per family: first = the smallest position among its genomes (a walk
//                                 over the CSR row of a family of s genomes where s * s <= G, else a walk along the order over
//                                 the family's bit row to the first set bit: G / s places on average), run = the leading
//                                 positions of the order whose genome holds the family (a walk along the order that stops at the
//                                 first clear bit — and does not start unless first == 0, so a unique family costs its one
//                                 position).  A family of all G genomes is first = 0, run = G without a walk.  Both into the LDS
//                                 bins, the bins that are not
//                                 empty into the order's global row: integer atomics only, so no value depends on an order of
//                                 additions.
//   C-curves   k_pan_finish       a workgroup per order: pan[i] = #{first <= i}, core[i] = F - #{run <= i}
#pragma once

#include "pdl_common.h"
#include "pdl_scan.h"
#include "pdl_sort.h"

#include <cstring>

// control words of a run (pdl_ctx::ProfileBufs::ctl, u64)
enum : size_t {
    PDL_PF_BAD = 0,         // P-check: ids out of range; C-check: order entries that break a permutation
    PDL_PF_INCIDENCES = 1,  // total of the incidence scan
    PDL_PF_FAMILIES = 2,    // total of the family scan
    PDL_PF_SCC = 3,         // families with spread = G = size
    PDL_PF_MAX_SIZE = 4,
    PDL_PF_FIRST_BAD = 5,   // C-check: the smallest failing order (starts at all ones)
    PDL_PF_WORDS = 6,
};

constexpr uint32_t PDL_PROFILE_MAX_GENOMES = 8192;      // spread_by_genome: (G + 1) * G words
constexpr uint32_t PAN_THREADS = 256, PAN_TILE = 2048;  // families of one workgroup of k_pan_curves
static_assert(PDL_PAN_MAX_GENOMES <= 65536 && 8 * (PDL_PAN_MAX_GENOMES + 1) + 4 * PDL_PAN_MAX_GENOMES <= 65536,
              "k_pan_curves: 16-bit positions, and its LDS within a workgroup's 64 KB");

__global__ __launch_bounds__(256) void k_prof_check(const uint32_t *fam, const uint32_t *gen, uint32_t n, uint32_t G, uint64_t *d_bad) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (fam[i] >= n || gen[i] >= G) atomicAdd(reinterpret_cast<unsigned long long *>(d_bad), 1ull);
}

__global__ __launch_bounds__(256) void k_prof_keys(const uint32_t *fam, const uint32_t *gen, uint32_t n, uint32_t gbits, uint64_t *keys, uint32_t *genome_genes) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = gen[i];
    keys[i] = (uint64_t) fam[i] << gbits | g;
    atomicAdd(genome_genes + g, 1u);
}

// heads of the (label, genome) runs: incidence `pre` starts at position j
struct ProfIncFlag {
    const uint64_t *keys;
    __device__ uint32_t operator()(uint64_t j) const { return (uint32_t) (j == 0 || keys[j] != keys[j - 1]); }
};
struct ProfIncApply {
    const uint64_t *keys; uint32_t gbits, n;
    uint32_t *inc_start, *inc_genome, *inc_label, *inc_of_pos;
    __device__ void operator()(uint64_t j, uint32_t f, uint32_t pre) const {
        if (f) {
            const uint64_t k = keys[j];
            inc_start[pre] = (uint32_t) j; inc_genome[pre] = (uint32_t) (k & ((1ull << gbits) - 1)); inc_label[pre] = (uint32_t) (k >> gbits);
            inc_of_pos[j] = pre;
        }
        if (j + 1 == n) inc_start[pre + f] = n;
    }
};
// heads of the label runs: family `pre` starts at position j, which is the head of an incidence as well
struct ProfFamFlag {
    const uint64_t *keys; uint32_t gbits;
    __device__ uint32_t operator()(uint64_t j) const { return (uint32_t) (j == 0 || (keys[j] >> gbits) != (keys[j - 1] >> gbits)); }
};
struct ProfFamApply {
    const uint64_t *keys; uint32_t gbits, n;
    const uint32_t *inc_of_pos; const uint64_t *d_incidences;
    uint32_t *fam_start, *label, *genome_off, *fam_of_label;
    __device__ void operator()(uint64_t j, uint32_t f, uint32_t pre) const {
        if (f) {
            const uint32_t lab = (uint32_t) (keys[j] >> gbits);
            fam_start[pre] = (uint32_t) j; label[pre] = lab; genome_off[pre] = inc_of_pos[j]; fam_of_label[lab] = pre;
        }
        if (j + 1 == n) { fam_start[pre + f] = n; genome_off[pre + f] = (uint32_t) *d_incidences; }
    }
};

__global__ __launch_bounds__(256) void k_prof_families(const uint32_t *fam_start, const uint32_t *genome_off, uint32_t n, uint32_t G, uint64_t *ctl, uint32_t *size,
                                                       uint32_t *spread, uint32_t *size_hist, uint32_t *spread_hist) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f >= n || f >= ctl[PDL_PF_FAMILIES]) return;
    const uint32_t sz = fam_start[f + 1] - fam_start[f], sp = genome_off[f + 1] - genome_off[f];
    size[f] = sz; spread[f] = sp;
    if (sz > n || sp > G) return;                  // (cannot be: the host checks the totals; no bin outside the histograms either way)
    atomicAdd(size_hist + sz, 1u); atomicAdd(spread_hist + sp, 1u);
    atomicMax(reinterpret_cast<unsigned long long *>(ctl + PDL_PF_MAX_SIZE), (unsigned long long) sz);
    if (sp == G && sz == G) atomicAdd(reinterpret_cast<unsigned long long *>(ctl + PDL_PF_SCC), 1ull);
}

// by_genome: spread_by_genome [(G + 1) * G]; cls: the genomes' genes in core | accessory | unique families, [3][G]
__global__ __launch_bounds__(256) void k_prof_incidences(const uint32_t *inc_start, const uint32_t *inc_genome, const uint32_t *inc_label, const uint32_t *fam_of_label,
                                                         const uint32_t *genome_off, uint32_t n, uint32_t G, const uint64_t *ctl, uint32_t *copies, uint32_t *by_genome,
                                                         uint32_t *cls) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || i >= ctl[PDL_PF_INCIDENCES]) return;
    const uint32_t cp = inc_start[i + 1] - inc_start[i], g = inc_genome[i], lab = inc_label[i];
    copies[i] = cp;
    if (g >= G || lab >= n) return;                // (cannot be: both were checked)
    const uint32_t f = fam_of_label[lab], sp = genome_off[f + 1] - genome_off[f];
    if (sp > G) return;
    atomicAdd(by_genome + (size_t) sp * G + g, 1u);
    if (sp == G) atomicAdd(cls + g, cp);
    if (sp == 1) atomicAdd(cls + 2 * (size_t) G + g, cp);
    if (sp != G && sp != 1) atomicAdd(cls + (size_t) G + g, cp);
}

void pdl_run_profile(pdl_ctx *c, const uint32_t *family_of, const uint32_t *genome_of, uint32_t N, uint32_t G, pdl_profile_result &out) {
    hipStream_t st = c->stream;
    out = pdl_profile_result{};
    if (N >= 0x7fffffffu) PDL_FAIL(PDL_ERR_UNSUPPORTED, "pdl_family_profile: 2^31 genes and more");
    if (G > PDL_PROFILE_MAX_GENOMES) PDL_FAIL(PDL_ERR_UNSUPPORTED, "pdl_family_profile: %u genomes, the per-genome spread table is kept for at most %u", G, PDL_PROFILE_MAX_GENOMES);
    pdl_ctx::ProfileBufs &b = c->pf;
    b.spans.start(st);
    pdl_ctl_ready(c);
    const size_t n4 = (size_t) N * sizeof(uint32_t);
    const size_t hist_words = (size_t) (G + 1) + (size_t) (G + 1) * G + 4 * (size_t) G;      // spread_hist | spread_by_genome | genes | core | accessory | unique
    b.ctl.alloc(PDL_PF_WORDS * sizeof(uint64_t));
    b.up_fam.alloc(n4); b.up_gen.alloc(n4);
    b.k_a.alloc(2 * n4); b.k_b.alloc(2 * n4); b.v_a.alloc(n4); b.v_b.alloc(n4);
    for (DevBuf *d : {&b.inc_start, &b.fam_start, &b.genome_off, &b.size_hist}) d->alloc(n4 + 4);
    for (DevBuf *d : {&b.inc_genome, &b.inc_label, &b.inc_of_pos, &b.label, &b.fam_of_label, &b.size, &b.spread, &b.copies}) d->alloc(n4);
    b.hist.alloc(hist_words * 4);
    uint64_t *ctl = b.ctl.as<uint64_t>();
    uint32_t *fam = b.up_fam.as<uint32_t>(), *gen = b.up_gen.as<uint32_t>();
    uint32_t *spread_hist = b.hist.as<uint32_t>(), *by_genome = spread_hist + (G + 1), *genome_genes = by_genome + (size_t) (G + 1) * G, *cls = genome_genes + G;
    PDL_HIP(hipMemcpyAsync(fam, family_of, n4, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(gen, genome_of, n4, hipMemcpyHostToDevice, st));

    b.spans.begin();
    PDL_HIP(hipMemsetAsync(ctl, 0, PDL_PF_WORDS * sizeof(uint64_t), st));
    hipLaunchKernelGGL(k_prof_check, grid256(N), dim3(256), 0, st, fam, gen, N, G, ctl + PDL_PF_BAD);
    const uint64_t bad = pdl_gate(c, b.spans, ctl + PDL_PF_BAD);
    if (bad) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_family_profile: %llu genes carry a label outside [0, %u) or a genome id outside [0, %u)", (unsigned long long) bad, N, G);
    PDL_HIP(hipMemsetAsync(b.hist.p, 0, hist_words * 4, st));
    PDL_HIP(hipMemsetAsync(b.size_hist.p, 0, n4 + 4, st));
    const uint32_t gbits = bit_length64(G - 1);
    uint64_t *k_in = b.k_a.as<uint64_t>(), *k_out = b.k_b.as<uint64_t>();
    uint32_t *v_in = b.v_a.as<uint32_t>(), *v_out = b.v_b.as<uint32_t>();
    hipLaunchKernelGGL(k_prof_keys, grid256(N), dim3(256), 0, st, fam, gen, N, gbits, k_in, genome_genes);
    PDL_HIP(hipGetLastError());
    pdl_sort_pairs<uint64_t, uint32_t>(c, k_in, k_out, v_in, v_out, N, gbits + bit_length64(N - 1), true, nullptr, 0, true);
    uint32_t *inc_start = b.inc_start.as<uint32_t>(), *inc_genome = b.inc_genome.as<uint32_t>(), *inc_label = b.inc_label.as<uint32_t>();
    uint32_t *inc_of_pos = b.inc_of_pos.as<uint32_t>(), *fam_start = b.fam_start.as<uint32_t>(), *label = b.label.as<uint32_t>();
    uint32_t *genome_off = b.genome_off.as<uint32_t>(), *fam_of_label = b.fam_of_label.as<uint32_t>();
    uint32_t *size = b.size.as<uint32_t>(), *spread = b.spread.as<uint32_t>(), *copies = b.copies.as<uint32_t>(), *size_hist = b.size_hist.as<uint32_t>();
    scan_and_apply(c, N, ProfIncFlag{k_out}, ProfIncApply{k_out, gbits, N, inc_start, inc_genome, inc_label, inc_of_pos}, ctl + PDL_PF_INCIDENCES);
    scan_and_apply(c, N, ProfFamFlag{k_out, gbits}, ProfFamApply{k_out, gbits, N, inc_of_pos, ctl + PDL_PF_INCIDENCES, fam_start, label, genome_off, fam_of_label},
                   ctl + PDL_PF_FAMILIES);
    hipLaunchKernelGGL(k_prof_families, grid256(N), dim3(256), 0, st, fam_start, genome_off, N, G, ctl, size, spread, size_hist, spread_hist);
    hipLaunchKernelGGL(k_prof_incidences, grid256(N), dim3(256), 0, st, inc_start, inc_genome, inc_label, fam_of_label, genome_off, N, G, ctl, copies, by_genome, cls);
    PDL_HIP(hipGetLastError());
    b.spans.end();
    {
        PinRead rd(c);
        const uint64_t *w = rd.add<uint64_t>(ctl, PDL_PF_WORDS);
        rd.sync();
        out.incidences = (uint32_t) w[PDL_PF_INCIDENCES]; out.families = (uint32_t) w[PDL_PF_FAMILIES];
        out.single_copy_core = (uint32_t) w[PDL_PF_SCC]; out.max_size = (uint32_t) w[PDL_PF_MAX_SIZE];
        if (w[PDL_PF_INCIDENCES] > N || w[PDL_PF_FAMILIES] > w[PDL_PF_INCIDENCES] || w[PDL_PF_FAMILIES] == 0 || w[PDL_PF_MAX_SIZE] > N || w[PDL_PF_MAX_SIZE] == 0)
            PDL_FAIL(PDL_ERR_DEVICE, "pdl_family_profile: inconsistent counts (%llu families, %llu incidences, largest family %llu of %u genes)",
                     (unsigned long long) w[PDL_PF_FAMILIES], (unsigned long long) w[PDL_PF_INCIDENCES], (unsigned long long) w[PDL_PF_MAX_SIZE], N);
    }
    out.n_sequences = N; out.n_genomes = G;
    const size_t F = out.families, Z = out.incidences;
    copy_down(st, out.label, label, F); copy_down(st, out.size, size, F); copy_down(st, out.spread, spread, F); copy_down(st, out.genome_off, genome_off, F + 1);
    copy_down(st, out.genomes, inc_genome, Z); copy_down(st, out.copies, copies, Z);
    copy_down(st, out.size_hist, size_hist, (size_t) out.max_size + 1); copy_down(st, out.hist, b.hist.p, hist_words);
    PDL_HIP(hipStreamSynchronize(st));
    const uint32_t *sh = out.hist.data();
    out.core = sh[G]; out.unique = sh[1];
    out.accessory = 0;
    for (uint32_t s = 2; s < G; s++) out.accessory += sh[s];
    out.device_ms = b.spans.total_ms();
}

// ---- the curves --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pan_check(const uint32_t *orders, uint32_t G, uint64_t *ctl) {
    __shared__ uint32_t s_seen[PDL_PAN_MAX_GENOMES / 32];
    __shared__ uint32_t s_bad;
    const uint32_t tid = threadIdx.x, o = blockIdx.x;
    if (tid < PDL_PAN_MAX_GENOMES / 32) s_seen[tid] = 0;
    if (tid == 0) s_bad = 0;
    pdl_sync();
    const uint32_t *ord = orders + (size_t) o * G;
    uint32_t bad = 0;
    for (uint32_t i = tid; i < G; i += 256) {
        const uint32_t g = ord[i];
        if (g >= G) { bad++; continue; }
        const uint32_t bit = 1u << (g & 31);
        if (atomicOr(&s_seen[g >> 5], bit) & bit) bad++;
    }
    if (bad) atomicAdd(&s_bad, bad);
    pdl_sync();
    if (tid == 0 && s_bad) {
        atomicAdd(reinterpret_cast<unsigned long long *>(ctl + PDL_PF_BAD), (unsigned long long) s_bad);
        atomicMin(reinterpret_cast<unsigned long long *>(ctl + PDL_PF_FIRST_BAD), (unsigned long long) o);
    }
}

// a wave per family; bits [F][W] cleared before
__global__ __launch_bounds__(256) void k_pan_bits(const uint32_t *genome_off, const uint32_t *genomes, uint32_t F, uint32_t W, unsigned long long *bits) {
    const uint32_t f = blockIdx.x * (256 / PDL_WAVE) + threadIdx.x / PDL_WAVE, lane = threadIdx.x & (PDL_WAVE - 1);
    if (f >= F) return;
    unsigned long long *row = bits + (size_t) f * W;
    for (uint32_t i = genome_off[f] + lane, e = genome_off[f + 1]; i < e; i += PDL_WAVE) {
        const uint32_t g = genomes[i];
        atomicOr(row + (g >> 6), 1ull << (g & 63));
    }
}

// hist: per order [2][G + 1], cleared before — families by `first`, then by `run`
__global__ __launch_bounds__(PAN_THREADS) void k_pan_curves(const uint32_t *orders, const uint32_t *genome_off, const uint32_t *genomes, const unsigned long long *bits,
                                                            uint32_t F, uint32_t G, uint32_t W, uint32_t tiles, uint32_t *hist) {
    extern __shared__ uint32_t s_pan[];
    uint32_t *s_first = s_pan, *s_run = s_pan + (G + 1);
    uint16_t *s_order = reinterpret_cast<uint16_t *>(s_pan + 2 * (size_t) (G + 1)), *s_pos = s_order + G;
    const uint32_t tid = threadIdx.x, o = blockIdx.x / tiles, t = blockIdx.x % tiles;
    const uint32_t *ord = orders + (size_t) o * G;
    for (uint32_t i = tid; i < G; i += PAN_THREADS) {
        const uint32_t g = ord[i];                 // (a permutation of 0..G-1: k_pan_check has seen to it)
        s_order[i] = (uint16_t) g; s_pos[g] = (uint16_t) i;
    }
    for (uint32_t i = tid; i <= G; i += PAN_THREADS) { s_first[i] = 0; s_run[i] = 0; }
    pdl_sync();
    const uint32_t f0 = t * PAN_TILE, f1 = F - f0 < PAN_TILE ? F : f0 + PAN_TILE;
    for (uint32_t f = f0 + tid; f < f1; f += PAN_THREADS) {
        const uint32_t a = genome_off[f], e = genome_off[f + 1];
        uint32_t first = G, run = 0;
        if (e - a == G) { first = 0; run = G; }
        else {
            const unsigned long long *row = bits + (size_t) f * W;
            const uint32_t sp = e - a;
            if ((uint64_t) sp * sp > G) {          // a wide family: the first set bit along the order comes after G / sp places on average, fewer than its sp genomes
                for (first = 0; first < G; first++) {
                    const uint32_t g = s_order[first];
                    if ((row[g >> 6] >> (g & 63)) & 1ull) break;
                }
            } else {
                for (uint32_t i = a; i < e; i++) { const uint32_t p = s_pos[genomes[i]]; first = p < first ? p : first; }
            }
            if (first == 0) {
                for (run = 1; run < G; run++) {
                    const uint32_t g = s_order[run];
                    if (!((row[g >> 6] >> (g & 63)) & 1ull)) break;
                }
            }
        }
        atomicAdd(s_first + first, 1u); atomicAdd(s_run + run, 1u);
    }
    pdl_sync();
    uint32_t *h = hist + (size_t) o * 2 * (G + 1);
    for (uint32_t i = tid; i <= G; i += PAN_THREADS) {
        const uint32_t a = s_first[i], r = s_run[i];
        if (a) atomicAdd(h + i, a);
        if (r) atomicAdd(h + (G + 1) + i, r);
    }
}

// a workgroup per order: the prefix sums of its two histograms, a thread per stretch of ceil(G / 256) bins, both sums in one word
__global__ __launch_bounds__(256) void k_pan_finish(const uint32_t *hist, uint32_t F, uint32_t G, uint32_t *pan, uint32_t *core) {
    __shared__ unsigned long long s_sum[256];
    const uint32_t tid = threadIdx.x, o = blockIdx.x;
    const uint32_t *hf = hist + (size_t) o * 2 * (G + 1), *hr = hf + (G + 1);
    const uint32_t chunk = (G + 255) / 256, i0 = tid * chunk < G ? tid * chunk : G, i1 = i0 + chunk < G ? i0 + chunk : G;
    unsigned long long own = 0;
    for (uint32_t i = i0; i < i1; i++) own += (unsigned long long) hf[i] << 32 | hr[i];        // (each half stays below 2^31: at most F families)
    s_sum[tid] = own;
    pdl_sync();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const unsigned long long v = tid >= d ? s_sum[tid - d] : 0ull;
        pdl_sync();
        s_sum[tid] += v;
        pdl_sync();
    }
    unsigned long long acc = s_sum[tid] - own;
    for (uint32_t i = i0; i < i1; i++) {
        acc += (unsigned long long) hf[i] << 32 | hr[i];
        pan[(size_t) o * G + i] = (uint32_t) (acc >> 32);
        core[(size_t) o * G + i] = F - (uint32_t) acc;
    }
}

// The profile's fields against each other, on the host, before anything of it is indexed by anything of it: what pdl_pan_curves and
// pdl_genome_matrix ask of a caller's profile (`who` names the call in the messages).  with_copies: the rows' copies and the sizes
// as well (no copy count of 0, a row's copies add up to its size, the sizes to n_sequences) -> the sum over the families of their
// largest copy count - 1 (pdl_matrix.h's extra bit columns); without: 0.
uint64_t pdl_check_profile(const pdl_profile *p, const char *who, bool with_copies) {
    const uint32_t G = p->n_genomes, F = p->families, Z = p->incidences;
    if (G == 0 || F == 0 || Z < F) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: a profile of %u genomes, %u families and %u incidences", who, G, F, Z);
    if (!p->genome_off || !p->genomes || !p->spread) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: the profile's genome_off, genomes or spread is NULL", who);
    if (with_copies && (!p->copies || !p->size)) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: the profile's copies or size is NULL", who);
    if (Z >= 0x7fffffffu) PDL_FAIL(PDL_ERR_UNSUPPORTED, "%s: 2^31 incidences and more", who);
    if (p->genome_off[0] != 0 || p->genome_off[F] != Z) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: the profile's genome_off runs from %u to %u, not from 0 to its %u incidences", who, p->genome_off[0], p->genome_off[F], Z);
    uint32_t n_core = 0;
    uint64_t extras = 0, genes = 0;
    for (uint32_t f = 0; f < F; f++) {
        const uint32_t a = p->genome_off[f], e = p->genome_off[f + 1];
        if (e <= a || e > Z || e - a > G || e - a != p->spread[f]) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: the profile's family %u has the row [%u, %u) and spread %u (%u genomes)", who, f, a, e, p->spread[f], G);
        for (uint32_t i = a; i < e; i++)
            if (p->genomes[i] >= G || (i > a && p->genomes[i] <= p->genomes[i - 1])) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: the profile's family %u names genome %u at place %u of its row (ascending ids below %u)", who, f, p->genomes[i], i - a, G);
        n_core += e - a == G;
        if (with_copies) {
            uint64_t sum = 0;
            uint32_t most = 0;
            for (uint32_t i = a; i < e; i++) {
                if (p->copies[i] == 0) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: the profile's family %u has 0 copies in genome %u", who, f, p->genomes[i]);
                sum += p->copies[i]; most = std::max(most, p->copies[i]);
            }
            if (sum != p->size[f]) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: the copies of the profile's family %u add up to %llu, its size is %u", who, f, (unsigned long long) sum, p->size[f]);
            extras += most - 1; genes += sum;
        }
    }
    if (n_core != p->core) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: the profile says %u core families, its rows hold %u", who, p->core, n_core);
    if (with_copies && genes != p->n_sequences) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: the sizes of the profile's families add up to %llu, it says %u genes", who, (unsigned long long) genes, p->n_sequences);
    return extras;
}

void pdl_run_pan_curves(pdl_ctx *c, const pdl_profile *p, const uint32_t *orders, uint32_t n_orders, pdl_curves_result &out) {
    hipStream_t st = c->stream;
    out = pdl_curves_result{};
    const uint32_t G = p->n_genomes, F = p->families, Z = p->incidences;
    pdl_check_profile(p, "pdl_pan_curves", false);
    if (G > PDL_PAN_MAX_GENOMES) PDL_FAIL(PDL_ERR_UNSUPPORTED, "pdl_pan_curves: %u genomes, the kernel's LDS holds an order of at most %u", G, (uint32_t) PDL_PAN_MAX_GENOMES);
    const uint64_t cells = (uint64_t) n_orders * G, tiles = (F + PAN_TILE - 1) / PAN_TILE, W = (G + 63) / 64;
    if (cells >= 0x7fffffffull || tiles * n_orders >= 0x7fffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "pdl_pan_curves: %u orders of %u genomes over %u families exceed 2^31 values or workgroups", n_orders, G, F);

    pdl_ctx::ProfileBufs &b = c->pf;
    b.spans.start(st);
    const size_t hist_bytes = (size_t) n_orders * 2 * (G + 1) * 4, bits_bytes = (size_t) F * W * 8;
    b.ctl.alloc(PDL_PF_WORDS * sizeof(uint64_t));
    b.up_orders.alloc(cells * 4); b.up_off.alloc(((size_t) F + 1) * 4); b.up_genomes.alloc((size_t) Z * 4);
    b.bits.alloc(bits_bytes); b.order_hist.alloc(hist_bytes); b.pan.alloc(cells * 4); b.core.alloc(cells * 4);
    uint64_t *ctl = b.ctl.as<uint64_t>();
    uint32_t *d_orders = b.up_orders.as<uint32_t>(), *d_off = b.up_off.as<uint32_t>(), *d_gen = b.up_genomes.as<uint32_t>();
    PDL_HIP(hipMemcpyAsync(d_orders, orders, cells * 4, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(d_off, p->genome_off, ((size_t) F + 1) * 4, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(d_gen, p->genomes, (size_t) Z * 4, hipMemcpyHostToDevice, st));

    b.spans.begin();
    PDL_HIP(hipMemsetAsync(ctl, 0, PDL_PF_WORDS * sizeof(uint64_t), st));
    PDL_HIP(hipMemsetAsync(ctl + PDL_PF_FIRST_BAD, 0xff, sizeof(uint64_t), st));
    hipLaunchKernelGGL(k_pan_check, dim3(n_orders), dim3(256), 0, st, d_orders, G, ctl);
    const uint64_t bad = pdl_gate(c, b.spans, ctl + PDL_PF_BAD);
    if (bad)            // (the refusal alone reads a second word)
        PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_pan_curves: order %llu is the first that is no permutation of 0..%u (%llu entries of the orders are %u and more or name a genome again)",
                 (unsigned long long) pdl_gate(c, ctl + PDL_PF_FIRST_BAD), G - 1, (unsigned long long) bad, G);
    PDL_HIP(hipMemsetAsync(b.bits.p, 0, bits_bytes, st));
    PDL_HIP(hipMemsetAsync(b.order_hist.p, 0, hist_bytes, st));
    unsigned long long *bits = b.bits.as<unsigned long long>();
    uint32_t *hist = b.order_hist.as<uint32_t>(), *pan = b.pan.as<uint32_t>(), *core = b.core.as<uint32_t>();
    hipLaunchKernelGGL(k_pan_bits, dim3((F + 3) / 4), dim3(256), 0, st, d_off, d_gen, F, (uint32_t) W, bits);
    const size_t lds = 8 * ((size_t) G + 1) + 4 * (size_t) G;
    hipLaunchKernelGGL(k_pan_curves, dim3((uint32_t) (tiles * n_orders)), dim3(PAN_THREADS), lds, st, d_orders, d_off, d_gen, bits, F, G, (uint32_t) W, (uint32_t) tiles, hist);
    hipLaunchKernelGGL(k_pan_finish, dim3(n_orders), dim3(256), 0, st, hist, F, G, pan, core);
    PDL_HIP(hipGetLastError());
    b.spans.end();
    out.n_genomes = G; out.n_orders = n_orders; out.families = F; out.incidences = Z;
    copy_down(st, out.pan, pan, cells); copy_down(st, out.core, core, cells);
    PDL_HIP(hipStreamSynchronize(st));
    out.device_ms = b.spans.total_ms();
}
