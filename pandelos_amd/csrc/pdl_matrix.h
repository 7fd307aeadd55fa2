// pdl_matrix.h — genome-by-genome shared-family matrices of a profile (pdl_genome_matrix); included at the end of pdl_bbh.hip.
// shared[g][h] = families with a gene in g and in h; shared_copies[g][h] = sum over the families of min(copies in g, copies in h),
// the multiset Jaccard's numerator one level above the k-mers.  min(a, b) = sum over t >= 1 of [a >= t] * [b >= t]: with the copy
// counts written in unary bit columns the min-sum is bilinear, and both matrices are AND-popcount products of one bit matrix.
//
//   M-extra    k_mx_extra         extra[f] = the largest copy count of family f's row - 1, a wave per family
//              scan_and_apply     extra_off = the exclusive scan of extra; its total E beside the host's own count
//   per slab of words [w0, w1) of the genomes' bit rows (G * (w1 - w0) * 8 bytes <= option "matrix_slab_bytes", cut at P / 64):
//   M-fill     k_mx_fill          the slab, cleared before, from the CSR: a wave per family, an incidence sets bit f (a presence
//                                 slab) or its run of copies - 1 bits from P + extra_off[f] (an extras slab), clipped to the slab
//   M-product  k_mx_product       one workgroup = a pair of 64-genome tiles (ti <= tj) and one k-split of the slab's words; both
//                                 tiles' words through LDS in steps of MX_KSTEP, 4 x 4 accumulators per thread, AND + popcount +
//                                 add per word pair; the sums onto the outputs by 32-bit integer atomics (both (g, h) and (h, g)
//                                 off the diagonal) — a presence slab into both matrices, an extras slab into shared_copies
//   M-out      the two matrices and E in one set of copies.
//
// Bit columns: P = 64 * ceil(F / 64) presence columns (bit f: family f has a gene in the genome), then E extra columns (bit
// P + extra_off[f] + t - 2: copies(f, g) >= t, t >= 2); L = P + E levels, W = ceil(L / 64) words per genome.  DESIGN.md section 21.
#pragma once

#include "pdl_common.h"
#include "pdl_scan.h"

// control words of a run (pdl_ctx::MatrixBufs::ctl, u64)
enum : size_t {
    PDL_MX_EXTRAS = 0,      // total of the scan over extra: E
    PDL_MX_WORDS = 1,
};

constexpr uint32_t MX_TILE = 64;            // genomes of one side of a workgroup's output tile
constexpr uint32_t MX_KSTEP = 16;           // 64-bit words of a genome staged per step
constexpr uint32_t MX_MIN_SPLIT_WORDS = 32; // a k-split keeps at least so many words (two steps) — but for the only one of a narrow slab
constexpr uint32_t MX_ROW = MX_TILE + 1;    // cells of one k-pair row of the LDS image: 64 genomes and one of padding (see k_mx_product)

// a wave per family
__global__ __launch_bounds__(256) void k_mx_extra(const uint32_t *genome_off, const uint32_t *copies, uint32_t F, uint32_t *extra) {
    const uint32_t f = blockIdx.x * (256 / PDL_WAVE) + threadIdx.x / PDL_WAVE, lane = threadIdx.x & (PDL_WAVE - 1);
    if (f >= F) return;
    uint32_t most = 1;
    for (uint32_t i = genome_off[f] + lane, e = genome_off[f + 1]; i < e; i += PDL_WAVE) { const uint32_t cp = copies[i]; most = cp > most ? cp : most; }
#pragma unroll
    for (int d = PDL_WAVE / 2; d > 0; d >>= 1) { const uint32_t o = __shfl_xor(most, d, PDL_WAVE); most = o > most ? o : most; }
    if (lane == 0) extra[f] = most - 1;
}

struct MxExtraFlag {
    const uint32_t *extra;
    __device__ uint32_t operator()(uint64_t f) const { return extra[f]; }
};
struct MxExtraApply {
    uint32_t *extra_off;
    __device__ void operator()(uint64_t f, uint32_t, uint32_t pre) const { extra_off[f] = pre; }
};

// a wave per family; bits [G][w1 - w0] cleared before.  presence: the slab lies below P / 64, else at or above it.
__global__ __launch_bounds__(256) void k_mx_fill(const uint32_t *genome_off, const uint32_t *genomes, const uint32_t *copies, const uint32_t *extra_off, uint32_t F,
                                                 uint32_t G, uint32_t P, uint32_t w0, uint32_t w1, int presence, unsigned long long *bits) {
    const uint32_t f = blockIdx.x * (256 / PDL_WAVE) + threadIdx.x / PDL_WAVE, lane = threadIdx.x & (PDL_WAVE - 1);
    if (f >= F) return;
    const uint32_t sw = w1 - w0;
    if (presence) {
        const uint32_t w = f >> 6;
        if (w < w0 || w >= w1) return;
        for (uint32_t i = genome_off[f] + lane, e = genome_off[f + 1]; i < e; i += PDL_WAVE) {
            const uint32_t g = genomes[i];
            if (g < G) atomicOr(bits + (size_t) g * sw + (w - w0), 1ull << (f & 63));
        }
        return;
    }
    const uint64_t first = (uint64_t) P + extra_off[f], lo = (uint64_t) w0 << 6, hi = (uint64_t) w1 << 6;
    if (first >= hi) return;
    for (uint32_t i = genome_off[f] + lane, e = genome_off[f + 1]; i < e; i += PDL_WAVE) {
        const uint32_t g = genomes[i], cp = copies[i];
        if (g >= G || cp < 2) continue;
        uint64_t a = first, z = first + (cp - 1);                      // the run of bits [a, z), clipped to the slab
        a = a < lo ? lo : a; z = z > hi ? hi : z;
        while (a < z) {
            const uint64_t stop = ((a >> 6) + 1) << 6, till = stop < z ? stop : z;       // the part of the run inside the word of a
            const uint32_t n = (uint32_t) (till - a);
            const unsigned long long mask = (n == 64 ? ~0ull : (1ull << n) - 1) << (a & 63);
            atomicOr(bits + (size_t) g * sw + ((a >> 6) - w0), mask);
            a = till;
        }
    }
}

// The product.  Workgroup = (pair of tiles, k-split): pair p = tj (tj + 1) / 2 + ti, ti <= tj; split s takes the slab's words
// [s * per, min(sw, (s + 1) * per)).  LDS image: per side [MX_KSTEP / 2][MX_ROW] cells of 16 bytes, k-pair-major — words 2 q and
// 2 q + 1 of the tile's genome r side by side in cell q * 65 + r.  Thread (ty, tx) = (tid / 16, tid % 16) holds the sums of rows
// ty + 16 a and columns tx + 16 b and reads a cell (two k) at a time.
//   reads (ds_read_b128, 64 banks of 4 bytes, four lane groups of 16 that each hold all 16 tx of parts of two ty): a row cell is one
//     address per ty (broadcast; the two ty of a group 16 bytes apart, other banks), the column cells of tx = 0..15 are 256
//     consecutive bytes, every bank once: no conflict, and 16 bytes per lane at the full 256 bytes per clock — as pairs of 8-byte
//     reads from a word-major image the compiler merges them into ds_read2_b64, which runs at half that rate;
//   writes (ds_write_b64, 32 banks, groups of 16 lanes): a group stages words k = 0..15 of ONE genome (128 consecutive bytes of
//     HBM): 8 cells 65 * 16 = 1040 bytes apart = 4 banks further per cell, 4 banks per cell: every bank once.  Without the pad
//     cell they would be 1024 bytes apart, all 8 on the same four banks.
// Genomes at and above G and words at and above the split's end are zeros in LDS; nothing is read past the slab.
__global__ __launch_bounds__(256) void k_mx_product(const unsigned long long *bits, uint32_t G, uint32_t sw, uint32_t per, uint32_t pairs, uint32_t *out_a,
                                                    uint32_t *out_b) {
    __shared__ ulonglong2 s_a[MX_KSTEP / 2 * MX_ROW], s_b[MX_KSTEP / 2 * MX_ROW];
    unsigned long long *w_a = reinterpret_cast<unsigned long long *>(s_a), *w_b = reinterpret_cast<unsigned long long *>(s_b);
    const uint32_t tid = threadIdx.x, p = blockIdx.x % pairs, s = blockIdx.x / pairs;
    uint32_t tj = (uint32_t) ((sqrtf(8.f * (float) p + 1.f) - 1.f) * 0.5f);
    while ((uint64_t) tj * (tj + 1) / 2 > p) tj--;
    while ((uint64_t) (tj + 1) * (tj + 2) / 2 <= p) tj++;
    const uint32_t ti = p - tj * (tj + 1) / 2;
    const uint32_t k0 = s * per, k1 = sw - k0 < per ? sw : k0 + per;
    const uint32_t ty = tid >> 4, tx = tid & 15;
    // staging: thread -> word kk of genome r0 + 16 q of the tile, q = 0..3
    const uint32_t kk = tid & (MX_KSTEP - 1), r0 = tid / MX_KSTEP;
    uint32_t acc[4][4] = {};
    unsigned long long pa[4], pb[4];
    const auto fetch = [&](uint32_t k) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t ga = ti * MX_TILE + r0 + 16 * q, gb = tj * MX_TILE + r0 + 16 * q;
            const bool in = k + kk < k1;
            pa[q] = in && ga < G ? bits[(size_t) ga * sw + k + kk] : 0ull;
            pb[q] = in && gb < G ? bits[(size_t) gb * sw + k + kk] : 0ull;
        }
    };
    fetch(k0);
    for (uint32_t k = k0; k < k1; k += MX_KSTEP) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t at = ((kk >> 1) * MX_ROW + r0 + 16 * q) * 2 + (kk & 1);
            w_a[at] = pa[q]; w_b[at] = pb[q];
        }
        pdl_sync();
        if (k + MX_KSTEP < k1) fetch(k + MX_KSTEP);                     // (uniform) the next step's words on their way during this one's sums
#pragma unroll 2
        for (uint32_t w = 0; w < MX_KSTEP / 2; w++) {
            ulonglong2 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; i++) { a[i] = s_a[w * MX_ROW + ty + 16 * i]; b[i] = s_b[w * MX_ROW + tx + 16 * i]; }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[i][j] += (uint32_t) __builtin_popcountll(a[i].x & b[j].x) + (uint32_t) __builtin_popcountll(a[i].y & b[j].y);
        }
        pdl_sync();
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t g = ti * MX_TILE + ty + 16 * i, h = tj * MX_TILE + tx + 16 * j, v = acc[i][j];
            if (g >= G || h >= G || v == 0) continue;
            atomicAdd(out_a + (size_t) g * G + h, v);
            if (out_b) atomicAdd(out_b + (size_t) g * G + h, v);
            if (ti != tj) {
                atomicAdd(out_a + (size_t) h * G + g, v);
                if (out_b) atomicAdd(out_b + (size_t) h * G + g, v);
            }
        }
}

void pdl_run_genome_matrix(pdl_ctx *c, const pdl_profile *p, pdl_matrix_result &out) {
    hipStream_t st = c->stream;
    out = pdl_matrix_result{};
    const uint64_t E = pdl_check_profile(p, "pdl_genome_matrix", true);
    const uint32_t G = p->n_genomes, F = p->families, Z = p->incidences;
    if (G > PDL_PROFILE_MAX_GENOMES) PDL_FAIL(PDL_ERR_UNSUPPORTED, "pdl_genome_matrix: %u genomes, the matrices are kept for at most %u", G, PDL_PROFILE_MAX_GENOMES);
    const uint64_t P = 64 * (((uint64_t) F + 63) / 64), L = P + E;
    if (L >= (1ull << 32)) PDL_FAIL(PDL_ERR_UNSUPPORTED, "pdl_genome_matrix: %llu bit columns, 2^32 and more", (unsigned long long) L);
    const uint32_t Pw = (uint32_t) (P / 64), W = (uint32_t) ((L + 63) / 64);
    const uint32_t slab_words = (uint32_t) std::min<uint64_t>(std::max<uint64_t>(c->opt_matrix_slab_bytes / ((uint64_t) G * 8), 1), W);
    const uint32_t tiles = (G + MX_TILE - 1) / MX_TILE, pairs = tiles * (tiles + 1) / 2;
    const size_t cells = (size_t) G * G;

    pdl_ctx::MatrixBufs &b = c->mx;
    b.spans.start(st);
    b.ctl.alloc(PDL_MX_WORDS * sizeof(uint64_t));
    b.up_off.alloc(((size_t) F + 1) * 4); b.up_genomes.alloc((size_t) Z * 4); b.up_copies.alloc((size_t) Z * 4);
    b.extra.alloc((size_t) F * 4); b.extra_off.alloc((size_t) F * 4);
    b.bits.alloc((size_t) G * slab_words * 8); b.shared.alloc(cells * 4); b.shared_copies.alloc(cells * 4);
    uint64_t *ctl = b.ctl.as<uint64_t>();
    uint32_t *d_off = b.up_off.as<uint32_t>(), *d_gen = b.up_genomes.as<uint32_t>(), *d_cp = b.up_copies.as<uint32_t>();
    uint32_t *extra = b.extra.as<uint32_t>(), *extra_off = b.extra_off.as<uint32_t>();
    uint32_t *shared = b.shared.as<uint32_t>(), *shared_copies = b.shared_copies.as<uint32_t>();
    unsigned long long *bits = b.bits.as<unsigned long long>();
    PDL_HIP(hipMemcpyAsync(d_off, p->genome_off, ((size_t) F + 1) * 4, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(d_gen, p->genomes, (size_t) Z * 4, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(d_cp, p->copies, (size_t) Z * 4, hipMemcpyHostToDevice, st));

    b.spans.begin();
    PDL_HIP(hipMemsetAsync(ctl, 0, PDL_MX_WORDS * sizeof(uint64_t), st));
    PDL_HIP(hipMemsetAsync(shared, 0, cells * 4, st));
    PDL_HIP(hipMemsetAsync(shared_copies, 0, cells * 4, st));
    hipLaunchKernelGGL(k_mx_extra, dim3((F + 3) / 4), dim3(256), 0, st, d_off, d_cp, F, extra);
    PDL_HIP(hipGetLastError());
    scan_and_apply(c, F, MxExtraFlag{extra}, MxExtraApply{extra_off}, ctl + PDL_MX_EXTRAS);
    const uint32_t want_grid = 2 * (uint32_t) pdl_cus(c);
    for (int presence = 1; presence >= 0; presence--) {
        const uint32_t from = presence ? 0 : Pw, to = presence ? Pw : W;
        for (uint32_t w0 = from; w0 < to; w0 += slab_words) {
            const uint32_t w1 = to - w0 < slab_words ? to : w0 + slab_words, sw = w1 - w0;
            // the k-splits: enough workgroups for twice the CUs while a split keeps MX_MIN_SPLIT_WORDS words; whole steps per split
            uint32_t splits = std::max(1u, std::min((want_grid + pairs - 1) / pairs, sw / MX_MIN_SPLIT_WORDS));
            const uint32_t per = ((sw + splits - 1) / splits + MX_KSTEP - 1) / MX_KSTEP * MX_KSTEP;
            splits = (sw + per - 1) / per;
            PDL_HIP(hipMemsetAsync(bits, 0, (size_t) G * sw * 8, st));
            hipLaunchKernelGGL(k_mx_fill, dim3((F + 3) / 4), dim3(256), 0, st, d_off, d_gen, d_cp, extra_off, F, G, (uint32_t) P, w0, w1, presence, bits);
            hipLaunchKernelGGL(k_mx_product, dim3(pairs * splits), dim3(256), 0, st, bits, G, sw, per, pairs, shared_copies, presence ? shared : nullptr);
            PDL_HIP(hipGetLastError());
            out.slabs++; out.splits = std::max(out.splits, splits);
        }
    }
    b.spans.end();
    std::vector<uint64_t> words;
    copy_down(st, words, ctl, PDL_MX_WORDS);
    copy_down(st, out.shared, shared, cells); copy_down(st, out.shared_copies, shared_copies, cells);
    PDL_HIP(hipStreamSynchronize(st));
    if (words[PDL_MX_EXTRAS] != E)
        PDL_FAIL(PDL_ERR_DEVICE, "pdl_genome_matrix: the device counted %llu extra bit columns, the host %llu", (unsigned long long) words[PDL_MX_EXTRAS], (unsigned long long) E);
    out.n_genomes = G; out.families = F; out.incidences = Z; out.levels = (uint32_t) L;
    out.device_ms = b.spans.total_ms();
}
