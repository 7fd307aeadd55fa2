// pdl_api.hip — the C ABI of include/pandelos_amd.h over the two device stages
// (pdl_dict.hip: preprocessSequences; pdl_join.hip: computeScores).
#include "pdl_common.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <limits>

static thread_local std::string g_create_error = "";

// Every entry point below has one shape: the NULL handles, the lock, then one `guarded` body (pdl_common.h) that opens with
// require_state(c, E_...) — the table of which entry point needs which state, and the reset pdl_stale, are pdl_state.h's.

// The argument checks on n new genes (residues, offsets [n + 1]): PDL_ERR_ARGUMENT
static void check_genes(const char *who, const uint8_t *residues, const uint64_t *offsets, uint32_t n) {
    if (!offsets) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: NULL pointer", who);
    if (n == 0) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: no gene", who);
    for (uint32_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: offsets decrease at gene %u", who, i);
    if (!residues && offsets[n] > offsets[0]) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: NULL residues", who);
}

// The argument checks on a batch of queries (gene_begin [n_queries + 1] cuts the n genes) and the 31-bit limit of every union:
// PDL_ERR_ARGUMENT, PDL_ERR_UNSUPPORTED
static void check_batch(const pdl_ctx *c, const char *who, const void *out, const uint8_t *residues, const uint64_t *offsets, const uint32_t *gene_begin,
                        uint32_t n, uint32_t n_queries) {
    if (n_queries == 0) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: no query", who);
    if (n == 0) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: no query gene", who);
    if (!out || !offsets || !gene_begin) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: NULL pointer", who);
    // gene_begin first: the 31-bit id limit is decided from it alone, before a single offset is read
    if (gene_begin[0] != 0) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: gene_begin[0] = %u, not 0", who, gene_begin[0]);
    for (uint32_t q = 0; q < n_queries; q++)
        if (gene_begin[q + 1] <= gene_begin[q] || gene_begin[q + 1] > n)
            PDL_FAIL(PDL_ERR_ARGUMENT, "%s: gene_begin is not strictly increasing within the %u genes at query %u (a query needs a gene)", who, n, q);
    if (gene_begin[n_queries] != n) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: gene_begin ends at %u, not at the %u genes", who, gene_begin[n_queries], n);
    for (uint32_t q = 0; q < n_queries; q++) {
        const uint64_t nc = (uint64_t) c->N + (gene_begin[q + 1] - gene_begin[q]);
        if (nc >= 0x7fffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "query %u: %llu genes in the union exceed the 31-bit gene ids", q, (unsigned long long) nc);
    }
    check_genes(who, residues, offsets, n);
}

template <class T> static T *xalloc(size_t n) {
    T *p = static_cast<T *>(malloc((n ? n : 1) * sizeof(T)));
    if (!p) throw std::bad_alloc();
    return p;
}
template <class T> static T *dup_vec(const std::vector<T> &v) {
    T *p = xalloc<T>(v.size());
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

extern "C" {

const char *pdl_version(void) { return "pandelos_amd 0.2 (HIP, gfx950)"; }

// The host side of the small-read protocol on plain memory (no device, no context): see PinRead in pdl_common.h.
int pdl_pin_arrived(const uint32_t *pin, const uint32_t *dst_word, const uint32_t *words, uint32_t n, uint32_t flag_word, uint32_t epoch) {
    if (!pin || !dst_word || !words) return -1;
    return pin_arrived(pin, dst_word, words, n, flag_word, epoch) ? 1 : 0;
}
uint32_t pdl_pin_checksum(const uint32_t *payload, const uint32_t *dst_word, const uint32_t *words, uint32_t n) {
    uint32_t sum = 0, at = 0;        // payload: the segments' words one after the other, as the kernel reads them from the device
    for (uint32_t s = 0; s < n; s++) for (uint32_t i = 0; i < words[s]; i++) sum += payload[at++] * pin_weight(dst_word[s] + i);
    return sum;
}

pdl_ctx *pdl_create(const pdl_config *cfg) {
    pdl_ctx *c = nullptr;
    guarded(nullptr, Lock::held, [&]() -> int {
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev == 0)
            PDL_FAIL(PDL_ERR_DEVICE, "no HIP device available (%s): pandelos_amd has no CPU path", hipGetErrorString(e));
        c = new pdl_ctx();
        int dev = cfg ? cfg->device : -1;
        if (dev < 0) PDL_HIP(hipGetDevice(&dev));
        if (dev >= ndev) PDL_FAIL(PDL_ERR_ARGUMENT, "device %d out of range (%d devices)", dev, ndev);
        c->device = dev;
        PDL_HIP(hipSetDevice(dev));
        c->flags = cfg ? cfg->flags : 0;
        if (cfg && cfg->stream) { c->stream = (hipStream_t) cfg->stream; c->own_stream = false; }
        else { PDL_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }
        // (coherent = fine-grained: what a kernel stores there is visible to the host while the kernel still runs — PinRead's flag)
        if (hipHostMalloc((void **) &c->pin, 1 << 20, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
            c->pin_bytes = 1 << 20; memset(c->pin + c->pin_bytes - PDL_PIN_FLAG_BYTES, 0, PDL_PIN_FLAG_BYTES);
            void *dp = nullptr;      // kernels store into the buffer through the device's alias of it, not through the host pointer
            if (hipHostGetDevicePointer(&dp, c->pin, 0) == hipSuccess && dp) c->pin_dev = static_cast<uint8_t *>(dp);
            else (void) hipGetLastError();
        } else { c->pin = nullptr; (void) hipGetLastError(); }
        return PDL_OK;
    }, [&] { delete c; c = nullptr; });
    return c;
}

void pdl_destroy(pdl_ctx *c) {
    if (!c) return;
    (void) hipSetDevice(c->device);
    (void) hipStreamSynchronize(c->stream);
    for (auto &e : c->ev) { if (e.a) (void) hipEventDestroy(e.a); if (e.b) (void) hipEventDestroy(e.b); }
    if (c->own_stream && c->stream) (void) hipStreamDestroy(c->stream);
    if (c->pin) (void) hipHostFree(c->pin);
    if (c->mirror) (void) hipHostFree(c->mirror);
    c->edge_mirror.release();
    if (c->task_pin) (void) hipHostFree(c->task_pin);
    if (c->ev_tasks) (void) hipEventDestroy(c->ev_tasks);
    if (c->ev_entry) (void) hipEventDestroy(c->ev_entry);
    if (c->copy_stream) (void) hipStreamDestroy(c->copy_stream);
    if (c->gen_pin) (void) hipHostFree(c->gen_pin);
    if (c->ev_gen) (void) hipEventDestroy(c->ev_gen);
    for (int i = 0; i < 2; i++) { if (c->ing_pin[i]) (void) hipHostFree(c->ing_pin[i]); if (c->ing_ev[i]) (void) hipEventDestroy(c->ing_ev[i]); }
    if (c->ing_stream) (void) hipStreamDestroy(c->ing_stream);
    delete c;                // (the work buffers and the span timers of the entry points go with their members)
}

const char *pdl_last_error(const pdl_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }

static void fill_cost(const pdl_ctx *c, pdl_cost *out) {
    if (!out) return;
    memset(out, 0, sizeof(*out));
    out->residues = c->R; out->kmer_occurrences = c->M; out->dictionary_records = c->U;
    out->shared_records = c->Ushared; out->groups = c->NG; out->total_cost = c->P;
    out->linear_ratio = c->sum_kseq ? (float) c->P / (float) c->sum_kseq : 0.f;   // library.cpp:350
    out->sequences = c->N; out->genomes = c->G; out->rank_base = c->rp.base; out->rank_bits = c->rp.rank_bits;
    out->hash_fallback = (int32_t) c->rp.hash_fallback; out->kvalue = (int32_t) c->rp.k;
}

// genome layout on the host: genome_sequences (library.cpp:244,268) as CSR
static void build_genome_layout(pdl_ctx *c) {
    const uint32_t N = c->N;
    uint32_t G = 0;
    for (uint32_t i = 0; i < N; i++) G = std::max(G, c->h_genome_of[i] + 1);      // library.cpp:242
    if ((uint64_t) G > (uint64_t) N) PDL_FAIL(PDL_ERR_ARGUMENT, "genome ids are not dense: max id %u with %u genes", G - 1, N);
    c->G = G;
    c->h_genome_row_off.assign((size_t) G + 1, 0);
    for (uint32_t i = 0; i < N; i++) c->h_genome_row_off[c->h_genome_of[i] + 1]++;
    for (uint32_t g = 0; g < G; g++) c->h_genome_row_off[g + 1] += c->h_genome_row_off[g];
    c->h_genome_rows.resize(N);
    std::vector<uint32_t> cur(c->h_genome_row_off.begin(), c->h_genome_row_off.end() - 1);
    for (uint32_t i = 0; i < N; i++) c->h_genome_rows[cur[c->h_genome_of[i]]++] = i;
}

// genome layout + what depends on the genome count (shard check)
static void layout_and_shard(pdl_ctx *c) {
    build_genome_layout(c);
    c->dict_shard.clear();
    if (c->shard_set) {
        for (uint32_t g : c->shard)
            if (g >= c->G) PDL_FAIL(PDL_ERR_ARGUMENT, "genome shard: id %u out of range (%u genomes)", g, c->G);
        c->dict_shard = c->shard;            // posting-range lists are built for these genomes' genes only
    }
}

}  // extern "C"   (C++ helpers of the other translation units)
// the two ends of device-resident offsets against n_res (a wrong n_res would make the ranking kernels read past the residues;
// ascending order is checked by K-len)
static void check_span(const uint64_t ends[2], uint64_t n_res) {
    if (ends[0] != 0 || ends[1] != n_res)
        PDL_FAIL(PDL_ERR_ARGUMENT, "offsets[0] = %llu, offsets[n] = %llu do not span the %llu residues", (unsigned long long) ends[0],
                 (unsigned long long) ends[1], (unsigned long long) n_res);
}
void pdl_input_arrived(pdl_ctx *c) {
    PDL_HIP(hipEventSynchronize(c->ev_gen));
    check_span(reinterpret_cast<const uint64_t *>(c->gen_pin + ((c->N + 1) & ~1u)), c->R);
}
void pdl_finish_layout(pdl_ctx *c) {
    c->h_genome_of.assign(c->gen_pin, c->gen_pin + c->N);
    c->layout_deferred = false;
    layout_and_shard(c);
}
void pdl_set_create_error(const std::string &msg) { g_create_error = msg; }
void pdl_extend_layout(pdl_ctx *c, const uint32_t *genome_ids, uint32_t n) {
    c->h_genome_of.insert(c->h_genome_of.end(), genome_ids, genome_ids + n);
    c->N += n;
    layout_and_shard(c);
}
void pdl_replace_layout(pdl_ctx *c, std::vector<uint32_t> &&genome_of) {
    c->h_genome_of = std::move(genome_of);
    c->N = (uint32_t) c->h_genome_of.size();
    layout_and_shard(c);
}

// What every build checks of its sizes, behind pdl_stale(Stale::set): a build refused here leaves a context that refuses every
// reader.  (The genome shard, if one was set, stays in force.)
static void begin_build(pdl_ctx *c, uint32_t n, uint64_t n_res, int k) {
    c->N = n; c->R = n_res;
    if (k <= 0) PDL_FAIL(PDL_ERR_KVALUE, "K value must be greater than 0.");
    if (n == 0) PDL_FAIL(PDL_ERR_EMPTY, "empty dataset");
}
// The common part of the single-GPU builds, behind the adopted input (d_res, d_off, d_gen; h_genome_of or the deferred layout)
void pdl_build(pdl_ctx *c, uint32_t n, uint64_t n_res, int k, int only_complexity, pdl_cost *out_cost) {
    PDL_HIP(hipSetDevice(c->device));
    pdl_stale(c, Stale::set);
    begin_build(c, n, n_res, k);
    if (!c->layout_deferred) layout_and_shard(c);        // (device input: done behind the first kernels, pdl_finish_layout)
    pdl_run_preprocess(c, k, only_complexity != 0);
    c->preprocessed = true;
    fill_cost(c, out_cost);
}

extern "C" {

// device-resident input: genome ids come to the host (task layout), and the two ends of the offsets are checked against n_res
static void adopt_device_input(pdl_ctx *c, const uint8_t *d_residues, const uint64_t *d_offsets, const uint32_t *d_genome_of,
                               uint32_t n, uint64_t n_res) {
    c->d_res = d_residues; c->d_off = d_offsets; c->d_gen = d_genome_of;
    c->h_genome_of.resize(n);
    uint64_t ends[2] = {0, n_res};
    if (n) {
        PDL_HIP(hipMemcpyAsync(c->h_genome_of.data(), d_genome_of, (size_t) n * 4, hipMemcpyDeviceToHost, c->stream));
        PDL_HIP(hipMemcpyAsync(&ends[0], d_offsets, 8, hipMemcpyDeviceToHost, c->stream));
        PDL_HIP(hipMemcpyAsync(&ends[1], d_offsets + n, 8, hipMemcpyDeviceToHost, c->stream));
    }
    PDL_HIP(hipStreamSynchronize(c->stream));
    check_span(ends, n_res);
}

int pdl_preprocess(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, const uint32_t *genome_of,
                   uint32_t n, int k, int only_complexity, pdl_cost *out_cost) {
    if (!c) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, [&]() -> int {
    if (!offsets || !genome_of || (!residues && n && offsets[n] > 0)) PDL_FAIL(PDL_ERR_ARGUMENT, "null input pointer");
    PDL_HIP(hipSetDevice(c->device));
    const uint64_t n_res = n ? offsets[n] - offsets[0] : 0;
    if (n && offsets[0] != 0) PDL_FAIL(PDL_ERR_ARGUMENT, "offsets[0] must be 0");
    c->in_res.alloc(n_res + 16); c->in_off.alloc(((size_t) n + 1) * 8); c->in_gen.alloc((size_t) n * 4 + 4);
    if (n_res) PDL_HIP(hipMemcpyAsync(c->in_res.p, residues, n_res, hipMemcpyHostToDevice, c->stream));
    PDL_HIP(hipMemcpyAsync(c->in_off.p, offsets, ((size_t) n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (n) PDL_HIP(hipMemcpyAsync(c->in_gen.p, genome_of, (size_t) n * 4, hipMemcpyHostToDevice, c->stream));
    c->d_res = c->in_res.as<uint8_t>(); c->d_off = c->in_off.as<uint64_t>(); c->d_gen = c->in_gen.as<uint32_t>();
    c->h_genome_of.assign(genome_of, genome_of + n);
    PDL_HIP(hipStreamSynchronize(c->stream));
    pdl_build(c, n, n_res, k, only_complexity, out_cost);
    return PDL_OK;
    });
}

int pdl_preprocess_device(pdl_ctx *c, const uint8_t *d_residues, const uint64_t *d_offsets, const uint32_t *d_genome_of,
                          uint32_t n, uint64_t n_res, int k, int only_complexity, pdl_cost *out_cost) {
    if (!c) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    const int rc = guarded(c, [&]() -> int {
    if (!d_offsets || !d_genome_of || (!d_residues && n_res)) PDL_FAIL(PDL_ERR_ARGUMENT, "null input pointer");
    if (((uintptr_t) d_residues & 15) != 0) PDL_FAIL(PDL_ERR_ARGUMENT, "d_residues must be 16-byte aligned");
    PDL_HIP(hipSetDevice(c->device));
    if (n == 0 || k <= 0) {
        adopt_device_input(c, d_residues, d_offsets, d_genome_of, n, n_res);
    } else {
        // genome ids and the two ends of the offsets start their way to the host (pinned: a true asynchronous copy); the
        // first kernels are queued behind them and the host builds the genome layout while those run
        c->d_res = d_residues; c->d_off = d_offsets; c->d_gen = d_genome_of;
        const size_t words = (((size_t) n + 1) & ~(size_t) 1) + 4;
        if (c->gen_pin_words < words) {
            if (c->gen_pin) (void) hipHostFree(c->gen_pin);
            c->gen_pin = nullptr; c->gen_pin_words = 0;
            PDL_HIP(hipHostMalloc((void **) &c->gen_pin, (words + words / 4) * sizeof(uint32_t), hipHostMallocDefault));
            c->gen_pin_words = words + words / 4;
        }
        if (!c->ev_gen) PDL_HIP(hipEventCreateWithFlags(&c->ev_gen, hipEventDisableTiming));
        uint64_t *ends = reinterpret_cast<uint64_t *>(c->gen_pin + (((size_t) n + 1) & ~(size_t) 1));
        // (on the side stream, behind whatever the caller's stream holds so far: the build's first kernels do not queue up
        //  behind three copies)
        if (!c->copy_stream) {
            PDL_HIP(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
            PDL_HIP(hipEventCreateWithFlags(&c->ev_tasks, hipEventDisableTiming));
        }
        if (!c->ev_entry) PDL_HIP(hipEventCreateWithFlags(&c->ev_entry, hipEventDisableTiming));
        PDL_HIP(hipEventRecord(c->ev_entry, c->stream));
        PDL_HIP(hipStreamWaitEvent(c->copy_stream, c->ev_entry, 0));
        PDL_HIP(hipMemcpyAsync(ends, d_offsets, 8, hipMemcpyDeviceToHost, c->copy_stream));
        PDL_HIP(hipMemcpyAsync(ends + 1, d_offsets + n, 8, hipMemcpyDeviceToHost, c->copy_stream));
        PDL_HIP(hipMemcpyAsync(c->gen_pin, d_genome_of, (size_t) n * 4, hipMemcpyDeviceToHost, c->copy_stream));
        PDL_HIP(hipEventRecord(c->ev_gen, c->copy_stream));
        c->layout_deferred = true;
    }
    pdl_build(c, n, n_res, k, only_complexity, out_cost);
    return PDL_OK;
    });
    c->layout_deferred = false;         // (whatever the call's end)
    return rc;
}

int pdl_genome_cost(const pdl_ctx *cc, uint32_t genome, uint64_t *out) {
    pdl_ctx *c = const_cast<pdl_ctx *>(cc);
    if (!c || !out) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, [&]() -> int {
    require_state(c, E_GENOME_COST);
    if (genome >= c->G) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_genome_cost: genome %u out of range (%u genomes)", genome, c->G);
    if (!c->costs_ready) {                       // (packed ranges: the per-gene / per-genome lookups are made on first request)
        PDL_HIP(hipSetDevice(c->device));
        pdl_ensure_costs(c);
    }
    *out = c->h_genome_cost[genome];
    return PDL_OK;
    });
}

int pdl_sequence_costs(const pdl_ctx *cc, uint64_t *out_cost, uint32_t *out_kseq) {
    pdl_ctx *c = const_cast<pdl_ctx *>(cc);
    if (!c || !out_cost) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, [&]() -> int {
    require_state(c, E_SEQUENCE_COSTS);
    PDL_HIP(hipSetDevice(c->device));
    pdl_ensure_costs(c);
    PDL_HIP(hipMemcpyAsync(out_cost, c->cost.p, (size_t) c->N * 8, hipMemcpyDeviceToHost, c->stream));
    if (out_kseq) PDL_HIP(hipMemcpyAsync(out_kseq, c->kseq_len.p, (size_t) c->N * 4, hipMemcpyDeviceToHost, c->stream));
    PDL_HIP(hipStreamSynchronize(c->stream));
    return PDL_OK;
    });
}

int pdl_set_genome_shard(pdl_ctx *c, const uint32_t *genomes, uint32_t count) {
    if (!c || (!genomes && count)) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, [&]() -> int {
    require_state(c, E_SET_GENOME_SHARD);
    std::vector<uint32_t> s(genomes, genomes + count);
    std::sort(s.begin(), s.end());
    for (size_t i = 0; i < s.size(); i++)
        if ((c->preprocessed && s[i] >= c->G) || (i && s[i] == s[i - 1])) PDL_FAIL(PDL_ERR_ARGUMENT, "genome shard: id out of range or repeated");
    // without a shard the ranges hold only the genes above each row and every cell is produced once for both
    // rows; scoring a subset needs the full ranges of a shard-aware build
    if (c->preprocessed && c->upper_only && count != 0 && s.size() != c->G)
        PDL_FAIL(PDL_ERR_STATE, "genome shard: set it before pdl_preprocess (the dictionary on the device was built for all genomes)");
    bool rebuild = false;
    if (c->preprocessed && !c->dict_shard.empty()) {
        // the dictionary on the device only has range lists for the genes of dict_shard: another shard gets its own before the next
        // scoring pass (the postings stay: two passes over them, pdl_run_reshard) — how a large set is scored a batch of genomes at a time
        if (count == 0) PDL_FAIL(PDL_ERR_STATE, "genome shard: the dictionary was built for a shard; run pdl_preprocess again to widen it to all genomes");
        for (uint32_t g : s)
            if (!std::binary_search(c->dict_shard.begin(), c->dict_shard.end(), g)) rebuild = true;
        if (rebuild && (c->only_complexity || !c->head_bits.p)) PDL_FAIL(PDL_ERR_STATE, "genome shard: not a subset of the shard the dictionary was built for; run pdl_preprocess again");
    }
    c->reshard_pending = c->reshard_pending || rebuild;
    c->shard = std::move(s);
    c->shard_set = count != 0;
    pdl_stale(c, Stale::scores_and_tasks);
    return PDL_OK;
    });
}

// The scoring pass, unless the context is scored (the caller holds the lock and a guard)
static void score_all_locked(pdl_ctx *c) {
    if (c->scored) return;
    require_state(c, E_SCORE);
    PDL_HIP(hipSetDevice(c->device));
    pdl_stale(c, Stale::scores);
    if (c->reshard_pending) { pdl_run_reshard(c); c->reshard_pending = false; }
    pdl_run_score_all(c);
}
// ... and `genome` is one of this context's
static void scored_and_mine(pdl_ctx *c, uint32_t genome) {
    score_all_locked(c);
    if (genome >= c->G) PDL_FAIL(PDL_ERR_ARGUMENT, "genome %u out of range (%u genomes)", genome, c->G);
    if (c->h_local_genome[genome] < 0) PDL_FAIL(PDL_ERR_ARGUMENT, "genome %u is not in this context's shard", genome);
}

int pdl_score_all(pdl_ctx *c) {
    if (!c) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, [&]() -> int { score_all_locked(c); return PDL_OK; });
}

int pdl_scores_counts(pdl_ctx *c, uint32_t *out) {
    if (!c || !out) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, [&]() -> int {
    score_all_locked(c);
    for (uint32_t g = 0; g < c->G; g++) {
        int32_t lg = c->h_local_genome[g];
        out[g] = lg < 0 ? 0u : (uint32_t) (c->h_cell_off[lg + 1] - c->h_cell_off[lg]);
    }
    return PDL_OK;
    });
}

void pdl_free_scores(pdl_scores *s) {
    if (!s) return;
    free(s->scores); free(s->percs); free(s->tr_percs); free(s->row); free(s->column);
    free(s->first_seq_genome); free(s->second_seq_genome); free(s->max_genome_score);
    free(s->max_genome_score_col); free(s->scoresMaxMappings);
    memset(s, 0, sizeof(*s));
}

// Device -> host copy for one calling thread, without the context lock: a stream and two pinned bounce buffers per
// thread (results beyond the host mirror's limit: the Java pool calls computeScores from ThreadsNum threads at once,
// Pangenes.java:54-66; the device arrays are immutable between scoring and the next preprocess).
namespace {
struct ThreadCopier {
    static constexpr size_t CHUNK = (size_t) 4 << 20;
    int device = -1;
    hipStream_t stream = nullptr;
    uint8_t *buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    void open(int dev) {
        if (device == dev && stream) return;
        close();
        PDL_HIP(hipSetDevice(dev));
        PDL_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        for (int i = 0; i < 2; i++) {
            PDL_HIP(hipHostMalloc((void **) &buf[i], CHUNK, hipHostMallocDefault));
            PDL_HIP(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        }
        device = dev;
    }
    void close() {
        for (int i = 0; i < 2; i++) { if (buf[i]) (void) hipHostFree(buf[i]); if (ev[i]) (void) hipEventDestroy(ev[i]); buf[i] = nullptr; ev[i] = nullptr; }
        if (stream) (void) hipStreamDestroy(stream);
        stream = nullptr; device = -1;
    }
    // dst (pageable) = src (device): chunk i+1 is in flight while chunk i is copied out of its bounce buffer
    void fetch(void *dst, const void *src, size_t bytes) {
        uint8_t *d = static_cast<uint8_t *>(dst);
        const uint8_t *sp = static_cast<const uint8_t *>(src);
        size_t issued = 0, drained = 0;
        int slot = 0;
        size_t len[2] = {0, 0};
        while (drained < bytes) {
            if (issued < bytes && (issued - drained) < 2 * CHUNK) {
                const size_t n = std::min(CHUNK, bytes - issued);
                PDL_HIP(hipMemcpyAsync(buf[slot], sp + issued, n, hipMemcpyDeviceToHost, stream));
                PDL_HIP(hipEventRecord(ev[slot], stream));
                len[slot] = n; issued += n; slot ^= 1;
                if (issued < bytes && issued - drained < 2 * CHUNK) continue;
            }
            const int dslot = (int) ((drained / CHUNK) & 1);
            PDL_HIP(hipEventSynchronize(ev[dslot]));
            memcpy(d + drained, buf[dslot], len[dslot]);
            drained += len[dslot];
        }
    }
    ~ThreadCopier() { close(); }
};
thread_local ThreadCopier t_copier;
}  // namespace

int pdl_compute_scores(pdl_ctx *c, uint32_t genome, pdl_scores *out) {
    if (!c || !out) return PDL_ERR_ARGUMENT;
    memset(out, 0, sizeof(*out));
    return guarded(c, Lock::take, [&]() -> int {
    bool use_mirror = false;
    size_t b_cells = 0, b_ms = 0;
    {
        // The lock covers the scoring pass (first call) and the one-time fill of the host mirror; slicing a genome's block
        // out of either the mirror or the device arrays runs without it, so the pool's threads do not serialise.
        std::lock_guard<std::mutex> lk(c->mu);
        scored_and_mine(c, genome);
        // Results up to PDL_MIRROR_LIMIT come to the host once, into pinned memory, with one copy per array; the per-genome
        // calls (the reference's thread pool makes G of them, Pangenes.java:54-66) then only slice that mirror.
        const uint64_t Zall = c->h_cell_off.back();
        const size_t S = c->shard.size();
        b_cells = (size_t) Zall * 4; b_ms = (size_t) c->n_task_rows * c->G * 4;
        const size_t b_cm = S * (size_t) c->N * 4;
        const size_t need = 5 * b_cells + b_ms + b_cm;
        constexpr size_t PDL_MIRROR_LIMIT = (size_t) 1 << 30;
        use_mirror = need <= PDL_MIRROR_LIMIT && c->opt_host_mirror;
        if (use_mirror && !c->mirror_valid) {
            PDL_HIP(hipSetDevice(c->device));
            hipStream_t st = c->stream;
            if (c->mirror_bytes < need) {
                if (c->mirror) { (void) hipHostFree(c->mirror); c->mirror = nullptr; c->mirror_bytes = 0; }
                PDL_HIP(hipHostMalloc((void **) &c->mirror, need + need / 4 + 64, hipHostMallocDefault));
                c->mirror_bytes = need + need / 4 + 64;
            }
            uint8_t *m = c->mirror;
            const void *src[5] = {c->c_score.p, c->c_perc.p, c->c_tr.p, c->c_row.p, c->c_col.p};
            for (int i = 0; i < 5; i++)
                if (b_cells) PDL_HIP(hipMemcpyAsync(m + (size_t) i * b_cells, src[i], b_cells, hipMemcpyDeviceToHost, st));
            if (b_ms) PDL_HIP(hipMemcpyAsync(m + 5 * b_cells, c->MS.p, b_ms, hipMemcpyDeviceToHost, st));
            if (b_cm) PDL_HIP(hipMemcpyAsync(m + 5 * b_cells + b_ms, c->CM.p, b_cm, hipMemcpyDeviceToHost, st));
            PDL_HIP(hipStreamSynchronize(st));
            c->mirror_valid = true;
        }
    }
    const int32_t lg = c->h_local_genome[genome];
    const uint32_t N = c->N, G = c->G;
    const uint64_t z0 = c->h_cell_off[lg], z1 = c->h_cell_off[lg + 1];
    const uint32_t z = (uint32_t) (z1 - z0);
    const uint32_t p0 = c->h_task_row_off[lg], rows = c->h_task_row_off[lg + 1] - p0;
    out->scoresCount = z; out->rows = rows; out->genomes = G; out->sequences = N;
    out->scores = xalloc<float>(z); out->percs = xalloc<float>(z); out->tr_percs = xalloc<float>(z);
    out->row = xalloc<int32_t>(z); out->column = xalloc<int32_t>(z);
    out->first_seq_genome = xalloc<int32_t>(z); out->second_seq_genome = xalloc<int32_t>(z);
    out->max_genome_score = xalloc<float>((size_t) rows * G);
    out->max_genome_score_col = xalloc<float>(N);
    out->scoresMaxMappings = xalloc<int32_t>(N);
    if (use_mirror) {
        const uint8_t *m = c->mirror;
        void *dst[5] = {out->scores, out->percs, out->tr_percs, out->row, out->column};
        for (int i = 0; i < 5; i++) if (z) memcpy(dst[i], m + (size_t) i * b_cells + (size_t) z0 * 4, (size_t) z * 4);
        if (rows) memcpy(out->max_genome_score, m + 5 * b_cells + (size_t) p0 * G * 4, (size_t) rows * G * 4);
        memcpy(out->max_genome_score_col, m + 5 * b_cells + b_ms + (size_t) lg * N * 4, (size_t) N * 4);
    } else {
        ThreadCopier &tc = t_copier;
        tc.open(c->device);
        if (z) {
            tc.fetch(out->scores, c->c_score.as<float>() + z0, (size_t) z * 4);
            tc.fetch(out->percs, c->c_perc.as<float>() + z0, (size_t) z * 4);
            tc.fetch(out->tr_percs, c->c_tr.as<float>() + z0, (size_t) z * 4);
            tc.fetch(out->row, c->c_row.as<int32_t>() + z0, (size_t) z * 4);
            tc.fetch(out->column, c->c_col.as<int32_t>() + z0, (size_t) z * 4);
        }
        if (rows) tc.fetch(out->max_genome_score, c->MS.as<float>() + (size_t) p0 * G, (size_t) rows * G * 4);
        tc.fetch(out->max_genome_score_col, c->CM.as<float>() + (size_t) lg * N, (size_t) N * 4);
    }
    // library.cpp:571-575: genome of row / column per cell;  :428-432: flat map
    for (uint32_t i = 0; i < z; i++) {
        out->first_seq_genome[i] = (int32_t) c->h_genome_of[out->row[i]];
        out->second_seq_genome[i] = (int32_t) c->h_genome_of[out->column[i]];
    }
    for (uint32_t i = 0; i < N; i++) out->scoresMaxMappings[i] = std::numeric_limits<int32_t>::max();
    for (uint32_t j = 0; j < rows; j++) out->scoresMaxMappings[c->h_genome_rows[c->h_genome_row_off[genome] + j]] = (int32_t) j;
    return PDL_OK;
    }, [&] { pdl_free_scores(out); });
}

void pdl_free_edges(pdl_edges *e) {
    if (!e) return;
    free(e->src); free(e->dst); free(e->score);
    memset(e, 0, sizeof(*e));
}

int pdl_compute_edges(pdl_ctx *c, uint32_t genome, pdl_edges *out) {
    if (!c || !out) return PDL_ERR_ARGUMENT;
    memset(out, 0, sizeof(*out));
    return guarded(c, Lock::take, [&]() -> int {
    {
        std::lock_guard<std::mutex> lk(c->mu);      // the scoring pass / the filter run once; slicing needs no lock
        scored_and_mine(c, genome);
        if (!c->edges_valid) {
            PDL_HIP(hipSetDevice(c->device));
            pdl_run_bbh_all(c);
        }
    }
    const int32_t lg = c->h_local_genome[genome];
    const uint64_t a1 = c->h_edge1[lg], b1 = c->h_edge1[lg + 1], a2 = c->h_edge_off[lg], b2 = c->h_edge_off[lg + 1];
    const uint64_t n1 = c->n_edges1, n2 = c->n_edges - c->n_edges1;
    const uint32_t cnt = (uint32_t) ((b1 - a1) + (b2 - a2));
    out->count = cnt;
    out->src = xalloc<int32_t>(cnt); out->dst = xalloc<int32_t>(cnt); out->score = xalloc<float>(cnt);
    const uint8_t *m = c->edge_mirror.p;
    const size_t k1 = (size_t) (b1 - a1), k2 = (size_t) (b2 - a2);
    if (k1) {
        memcpy(out->src, m + a1 * 4, k1 * 4); memcpy(out->dst, m + n1 * 4 + a1 * 4, k1 * 4); memcpy(out->score, m + n1 * 8 + a1 * 4, k1 * 4);
    }
    if (k2) {
        const uint8_t *m2 = m + n1 * 12;
        memcpy(out->src + k1, m2 + a2 * 4, k2 * 4); memcpy(out->dst + k1, m2 + n2 * 4 + a2 * 4, k2 * 4); memcpy(out->score + k1, m2 + n2 * 8 + a2 * 4, k2 * 4);
    }
    return PDL_OK;
    }, [&] { pdl_free_edges(out); });
}

// ---- K-fam (pdl_families.h) -------------------------------------------------------------------------------------------------
void pdl_free_families(pdl_families *f) {
    if (!f) return;
    free(f->component_of); free(f->is_node); free(f->family_off); free(f->family_genes); free(f->collides);
    memset(f, 0, sizeof(*f));
}

static void fill_families(const pdl_fam_result &r, pdl_families *out) {
    out->sequences = r.sequences; out->nodes = r.nodes; out->families = r.families; out->colliding = r.colliding; out->device_ms = r.device_ms;
    out->component_of = dup_vec(r.component_of); out->is_node = dup_vec(r.is_node); out->family_off = dup_vec(r.family_off);
    out->family_genes = dup_vec(r.family_genes); out->collides = dup_vec(r.collides);
}

// the context's families, computed on first use: scored, then the edges, then the families (the device is the context's then)
static void families_ready_locked(pdl_ctx *c) {
    score_all_locked(c);
    PDL_HIP(hipSetDevice(c->device));
    if (!c->edges_valid) pdl_run_bbh_all(c);
    if (!c->fam_valid) pdl_run_families_of_context(c);
}

int pdl_compute_families(pdl_ctx *c, pdl_families *out) {
    if (!c || !out) return PDL_ERR_ARGUMENT;
    memset(out, 0, sizeof(*out));
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, Lock::held, [&]() -> int {
        require_state(c, E_COMPUTE_FAMILIES);
        families_ready_locked(c);
        fill_families(c->fam, out);
        return PDL_OK;
    }, [&] { c->fam_valid = false; pdl_free_families(out); });      // (the families are made again by the next call: it costs a run, never an answer)
}

int pdl_families_of_edges(pdl_ctx *c, const int32_t *src, const int32_t *dst, uint64_t n_edges, const uint32_t *genome_of, uint32_t n_sequences,
                          pdl_families *out) {
    if (!c || !out) return PDL_ERR_ARGUMENT;
    memset(out, 0, sizeof(*out));
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, Lock::held, [&]() -> int {
        if ((n_edges && (!src || !dst)) || (n_sequences && !genome_of)) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_families_of_edges: NULL pointer");
        if (n_edges >= 0x7fffffffull || n_sequences >= 0x7fffffffu) PDL_FAIL(PDL_ERR_UNSUPPORTED, "pdl_families_of_edges: 2^31 genes or edges and more");
        PDL_HIP(hipSetDevice(c->device));
        pdl_ctx::FamBufs &b = c->fb;
        uint32_t g_max = 0;
        for (uint32_t i = 0; i < n_sequences; i++) g_max = std::max(g_max, genome_of[i]);
        if (n_edges) {
            b.up_src.alloc(n_edges * 4); b.up_dst.alloc(n_edges * 4);
            PDL_HIP(hipMemcpyAsync(b.up_src.p, src, n_edges * 4, hipMemcpyHostToDevice, c->stream));
            PDL_HIP(hipMemcpyAsync(b.up_dst.p, dst, n_edges * 4, hipMemcpyHostToDevice, c->stream));
        }
        if (n_sequences) {
            b.up_gen.alloc((size_t) n_sequences * 4);
            PDL_HIP(hipMemcpyAsync(b.up_gen.p, genome_of, (size_t) n_sequences * 4, hipMemcpyHostToDevice, c->stream));
        }
        const int32_t *s2[2] = {b.up_src.as<int32_t>(), nullptr}, *d2[2] = {b.up_dst.as<int32_t>(), nullptr};
        const uint64_t n2[2] = {n_edges, 0};
        pdl_fam_result r;
        pdl_run_families(c, s2, d2, n2, false, true, true, b.up_gen.as<uint32_t>(), n_sequences, bit_length64(g_max), r);
        fill_families(r, out);
        return PDL_OK;
    }, [&] { pdl_free_families(out); });
}

// ---- K-split (pdl_split.h) ---------------------------------------------------------------------------------------------------
void pdl_free_split(pdl_split *s) {
    if (!s) return;
    free(s->removed_off); free(s->removed_u); free(s->removed_v);
    memset(s, 0, sizeof(*s));
}

int pdl_split_first_level(pdl_ctx *c, uint32_t n_graphs, const uint64_t *node_off, const uint64_t *adj_off, const uint32_t *adj, pdl_split *out) {
    if (!c || !out) return PDL_ERR_ARGUMENT;
    memset(out, 0, sizeof(*out));
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, Lock::held, [&]() -> int {
        if (n_graphs == 0) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_split_first_level: no graph");
        if (!node_off || !adj_off) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_split_first_level: NULL pointer");
        PDL_HIP(hipSetDevice(c->device));
        pdl_split_result r;
        pdl_run_split(c, n_graphs, node_off, adj_off, adj, r);
        out->graphs = r.graphs; out->chunks = r.chunks; out->nodes = r.nodes; out->edges = r.edges;
        out->removals = r.removed_u.size(); out->rounds = r.rounds; out->device_ms = r.device_ms;
        out->removed_off = dup_vec(r.removed_off); out->removed_u = dup_vec(r.removed_u); out->removed_v = dup_vec(r.removed_v);
        return PDL_OK;
    }, [&] { pdl_free_split(out); });
}

// ---- Pan-genome profile (pdl_profile.h) -------------------------------------------------------------------------------------
void pdl_free_profile(pdl_profile *p) {
    if (!p) return;
    free(p->label); free(p->size); free(p->spread); free(p->genome_off); free(p->genomes); free(p->copies);
    free(p->size_hist); free(p->spread_hist); free(p->spread_by_genome);
    free(p->genome_genes); free(p->genome_core); free(p->genome_accessory); free(p->genome_unique);
    memset(p, 0, sizeof(*p));
}

int pdl_family_profile(pdl_ctx *c, const uint32_t *family_of, const uint32_t *genome_of, uint32_t n_sequences, uint32_t n_genomes, pdl_profile *out) {
    if (!c || !out) return PDL_ERR_ARGUMENT;
    memset(out, 0, sizeof(*out));
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, Lock::held, [&]() -> int {
        if (!family_of || !genome_of) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_family_profile: NULL pointer");
        if (n_sequences == 0 || n_genomes == 0) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_family_profile: %u genes in %u genomes", n_sequences, n_genomes);
        PDL_HIP(hipSetDevice(c->device));
        pdl_profile_result r;
        pdl_run_profile(c, family_of, genome_of, n_sequences, n_genomes, r);
        const size_t G = n_genomes;
        const auto part = [&](size_t at, size_t n) { return std::vector<uint32_t>(r.hist.begin() + at, r.hist.begin() + at + n); };
        out->n_sequences = r.n_sequences; out->n_genomes = r.n_genomes; out->families = r.families; out->incidences = r.incidences; out->max_size = r.max_size;
        out->core = r.core; out->single_copy_core = r.single_copy_core; out->unique = r.unique; out->accessory = r.accessory; out->device_ms = r.device_ms;
        out->label = dup_vec(r.label); out->size = dup_vec(r.size); out->spread = dup_vec(r.spread);
        out->genome_off = dup_vec(r.genome_off); out->genomes = dup_vec(r.genomes); out->copies = dup_vec(r.copies);
        out->size_hist = dup_vec(r.size_hist); out->spread_hist = dup_vec(part(0, G + 1)); out->spread_by_genome = dup_vec(part(G + 1, (G + 1) * G));
        const size_t per_genome = (G + 1) + (G + 1) * G;
        out->genome_genes = dup_vec(part(per_genome, G)); out->genome_core = dup_vec(part(per_genome + G, G));
        out->genome_accessory = dup_vec(part(per_genome + 2 * G, G)); out->genome_unique = dup_vec(part(per_genome + 3 * G, G));
        return PDL_OK;
    }, [&] { pdl_free_profile(out); });
}

void pdl_free_curves(pdl_curves *p) {
    if (!p) return;
    free(p->pan); free(p->core);
    memset(p, 0, sizeof(*p));
}

int pdl_pan_curves(pdl_ctx *c, const pdl_profile *profile, const uint32_t *orders, uint32_t n_orders, pdl_curves *out) {
    if (!c || !out) return PDL_ERR_ARGUMENT;
    memset(out, 0, sizeof(*out));
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, Lock::held, [&]() -> int {
        if (!profile || !orders) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_pan_curves: NULL pointer");
        if (n_orders == 0) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_pan_curves: no order");
        PDL_HIP(hipSetDevice(c->device));
        pdl_curves_result r;
        pdl_run_pan_curves(c, profile, orders, n_orders, r);
        out->n_genomes = r.n_genomes; out->n_orders = r.n_orders; out->families = r.families; out->incidences = r.incidences; out->device_ms = r.device_ms;
        out->pan = dup_vec(r.pan); out->core = dup_vec(r.core);
        return PDL_OK;
    }, [&] { pdl_free_curves(out); });
}

// ---- Genome-by-genome shared-family matrices (pdl_matrix.h) -----------------------------------------------------------------
void pdl_free_genome_matrix(struct pdl_genome_matrix *m) {
    if (!m) return;
    free(m->shared); free(m->shared_copies);
    memset(m, 0, sizeof(*m));
}

int pdl_genome_matrix(pdl_ctx *c, const pdl_profile *profile, struct pdl_genome_matrix *out) {
    if (out) memset(out, 0, sizeof(*out));
    if (!c || !out) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, Lock::held, [&]() -> int {
        if (!profile) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_genome_matrix: NULL pointer");
        PDL_HIP(hipSetDevice(c->device));
        pdl_matrix_result r;
        pdl_run_genome_matrix(c, profile, r);
        out->n_genomes = r.n_genomes; out->families = r.families; out->incidences = r.incidences; out->levels = r.levels;
        out->slabs = r.slabs; out->splits = r.splits; out->device_ms = r.device_ms;
        out->shared = dup_vec(r.shared); out->shared_copies = dup_vec(r.shared_copies);
        return PDL_OK;
    }, [&] { pdl_free_genome_matrix(out); });
}

// ---- K-place (pdl_place.h) ---------------------------------------------------------------------------------------------------
void pdl_free_placement(pdl_placement *p) {
    if (!p) return;
    free(p->src); free(p->dst); free(p->score); free(p->family_of); free(p->is_node); free(p->group_label); free(p->group_query_off);
    free(p->group_query); free(p->group_base_off); free(p->group_base); free(p->group_collides);
    memset(p, 0, sizeof(*p));
}

// (a query's edges are the C arrays themselves: they change hands)
static void fill_placement(pdl_place_result &r, bool with_edges, pdl_placement *out) {
    out->sequences = r.sequences; out->n_query = r.n_query; out->genomes = r.genomes;
    out->edges = (uint32_t) r.c_edges.n; out->edges_phase1 = r.edges_phase1; out->groups = r.groups;
    out->novel = r.novel; out->joined = r.joined; out->bridging = r.bridging; out->colliding = r.colliding; out->unplaced = r.unplaced;
    out->device_ms = r.device_ms;
    if (with_edges) { out->src = r.c_edges.src; out->dst = r.c_edges.dst; out->score = r.c_edges.score; r.c_edges.release(); }
    out->family_of = dup_vec(r.family_of); out->is_node = dup_vec(r.is_node); out->group_label = dup_vec(r.group_label);
    out->group_query_off = dup_vec(r.group_query_off); out->group_query = dup_vec(r.group_query);
    out->group_base_off = dup_vec(r.group_base_off); out->group_base = dup_vec(r.group_base); out->group_collides = dup_vec(r.group_collides);
}

// pdl_get_query_rekey_info's and pdl_get_query_join_info's books over one call of the four that score a query: opened behind the
// call's refusals of state and argument, closed — the reports become the context's — only when the call went through.
static void query_rekey_open(pdl_ctx *c) {
    c->qj_call = pdl_query_join_info{};
    c->qrk_call = pdl_query_rekey_info{};
    c->qrk_call.letters_base = c->qrk_call.letters_max = c->rp.base;
    c->qrk_call.key_bits_base = c->qrk_call.key_bits_max = c->rp.rank_bits;
}
static void query_rekey_close(pdl_ctx *c) { c->last_query_rekey = c->qrk_call; c->last_query_join = c->qj_call; }

int pdl_place_query(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, uint32_t n_query, pdl_placement *out, pdl_query_info *info) {
    if (!c) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    if (out) memset(out, 0, sizeof(*out));
    if (info) memset(info, 0, sizeof(*info));
    return guarded(c, Lock::held, [&]() -> int {
        require_state(c, E_PLACE_QUERY);
        if (!out) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_place_query: NULL pointer");
        check_genes("pdl_place_query", residues, offsets, n_query);
        families_ready_locked(c);
        pdl_place_result r;
        pdl_query_info qi{};
        query_rekey_open(c);
        pdl_run_place_query(c, residues, offsets, n_query, r, &qi);
        query_rekey_close(c);
        fill_placement(r, true, out);
        if (info) *info = qi;
        return PDL_OK;
    }, [&] { if (out) pdl_free_placement(out); if (info) memset(info, 0, sizeof(*info)); });
}

// A caller's base families behind their checks, on the device (c->pb.up through pdl_upload_base, the one upload of base families; up_gen, up_src, up_dst) with n_edges edges of the caller's: what
// pdl_placement_of_edges and its batch form share.  The base is indexed by its own fields on the device: they must be what K-fam
// writes (labels are smallest members, families in label order, members ascending, every node in exactly one family).
static void check_base_pointers(const char *who, const pdl_families *base, const uint32_t *genome_of, const int32_t *src, const int32_t *dst, uint64_t n_edges) {
    if (!base || (n_edges && (!src || !dst))) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: NULL pointer", who);
    const uint32_t N = base->sequences, F = base->families, nodes = base->nodes;
    if (N && (!genome_of || !base->component_of || !base->is_node)) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: NULL pointer", who);
    if (!base->family_off || (nodes && !base->family_genes) || (F && !base->collides)) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: NULL pointer in the base families", who);
}
static PlaceBase upload_base(pdl_ctx *c, const char *who, const pdl_families *base, const uint32_t *genome_of, const int32_t *src, const int32_t *dst, uint64_t n_edges) {
    const uint32_t N = base->sequences, F = base->families, nodes = base->nodes;
    if (nodes > N || F > nodes || base->family_off[0] != 0 || base->family_off[F] != nodes) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: inconsistent base families (counts)", who);
    std::vector<uint8_t> listed(N, 0);             // the gene is a member of exactly one family
    for (uint32_t f = 0; f < F; f++) {
        const uint32_t a = base->family_off[f], b = base->family_off[f + 1];
        if (b <= a || b > nodes) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: inconsistent base families (family_off at %u)", who, f);
        const uint32_t label = base->family_genes[a];
        if (f && label <= base->family_genes[base->family_off[f - 1]])
            PDL_FAIL(PDL_ERR_ARGUMENT, "%s: inconsistent base families (family %u is not behind family %u in label order)", who, f, f - 1);
        for (uint32_t j = a; j < b; j++) {
            const uint32_t g = base->family_genes[j];
            if (g >= N || listed[g] || !base->is_node[g] || base->component_of[g] != label || (j > a && g <= base->family_genes[j - 1]))
                PDL_FAIL(PDL_ERR_ARGUMENT, "%s: inconsistent base families (member %u of family %u)", who, j - a, f);
            listed[g] = 1;
        }
    }
    uint32_t g_max = 0;
    for (uint32_t i = 0; i < N; i++) {
        g_max = std::max(g_max, genome_of[i]);
        // a node is listed in a family (its component_of was checked there: a label below N); any other gene is its own component
        if (base->is_node[i] ? !listed[i] : base->component_of[i] != i)
            PDL_FAIL(PDL_ERR_ARGUMENT, "%s: inconsistent base families (gene %u)", who, i);
    }
    if (g_max >= 0x7fffffffu) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: genome id %u (ids below 2^31 - 1)", who, g_max);
    PDL_HIP(hipSetDevice(c->device));
    pdl_ctx::PlaceBufs &b = c->pb;
    hipStream_t st = c->stream;
    b.up_gen.alloc((size_t) N * 4);
    if (N) PDL_HIP(hipMemcpyAsync(b.up_gen.p, genome_of, (size_t) N * 4, hipMemcpyHostToDevice, st));
    if (n_edges) {
        b.up_src.alloc(n_edges * 4); b.up_dst.alloc(n_edges * 4);
        PDL_HIP(hipMemcpyAsync(b.up_src.p, src, n_edges * 4, hipMemcpyHostToDevice, st));
        PDL_HIP(hipMemcpyAsync(b.up_dst.p, dst, n_edges * 4, hipMemcpyHostToDevice, st));
    }
    return pdl_upload_base(c, FamView{N, F, nodes, base->component_of, base->family_off, base->family_genes, base->is_node, base->collides}, b.up,
                           b.up_gen.as<uint32_t>(), N ? g_max + 1 : 0);
}

int pdl_placement_of_edges(pdl_ctx *c, const pdl_families *base, const uint32_t *genome_of, uint32_t n_query, const int32_t *src, const int32_t *dst,
                           uint64_t n_edges, pdl_placement *out) {
    if (!c || !out) return PDL_ERR_ARGUMENT;
    memset(out, 0, sizeof(*out));
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, Lock::held, [&]() -> int {
        check_base_pointers("pdl_placement_of_edges", base, genome_of, src, dst, n_edges);
        if (n_query == 0) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_placement_of_edges: no query gene");
        if (n_edges >= 0x7fffffffull || (uint64_t) base->sequences + n_query >= 0x7fffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "pdl_placement_of_edges: 2^31 genes or edges and more");
        const PlaceBase B = upload_base(c, "pdl_placement_of_edges", base, genome_of, src, dst, n_edges);
        pdl_ctx::PlaceBufs &b = c->pb;
        pdl_place_result r;
        pdl_run_place_edges(c, B, n_query, b.up_src.as<int32_t>(), b.up_dst.as<int32_t>(), n_edges, r);
        fill_placement(r, false, out);
        return PDL_OK;
    }, [&] { pdl_free_placement(out); });
}

int pdl_place_batch(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, const uint32_t *gene_begin, uint32_t n, uint32_t n_queries,
                    pdl_placement *out, pdl_query_info *info, pdl_place_batch_info *binfo) {
    if (!c) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    if (out && n_queries) memset(out, 0, sizeof(*out) * (size_t) n_queries);
    if (info && n_queries) memset(info, 0, sizeof(*info) * (size_t) n_queries);
    if (binfo) memset(binfo, 0, sizeof(*binfo));
    return guarded(c, Lock::held, [&]() -> int {
        require_state(c, E_PLACE_BATCH);
        check_batch(c, "pdl_place_batch", out, residues, offsets, gene_begin, n, n_queries);
        families_ready_locked(c);
        std::vector<pdl_place_result> r;
        std::vector<pdl_query_info> qi(n_queries);
        uint32_t chunks = 0;
        float device_ms = 0.f;
        query_rekey_open(c);
        pdl_run_place_batch(c, residues, offsets, gene_begin, n, n_queries, r, qi.data(), &chunks, &device_ms);
        query_rekey_close(c);
        for (uint32_t q = 0; q < n_queries; q++) fill_placement(r[q], true, &out[q]);      // (only now: every chunk is through)
        if (info) memcpy(info, qi.data(), sizeof(*info) * (size_t) n_queries);
        if (binfo) { binfo->queries = n_queries; binfo->chunks = chunks; binfo->device_ms = device_ms; }
        return PDL_OK;
    }, [&] {
        if (out) for (uint32_t q = 0; q < n_queries; q++) pdl_free_placement(&out[q]);
        if (info && n_queries) memset(info, 0, sizeof(*info) * (size_t) n_queries);
        if (binfo) memset(binfo, 0, sizeof(*binfo));
    });
}

int pdl_placement_batch_of_edges(pdl_ctx *c, const pdl_families *base, const uint32_t *genome_of, uint32_t n_queries, const uint32_t *n_query,
                                 const uint64_t *edge_begin, const int32_t *src, const int32_t *dst, pdl_placement *out) {
    if (!c) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    if (out && n_queries) memset(out, 0, sizeof(*out) * (size_t) n_queries);
    return guarded(c, Lock::held, [&]() -> int {
        const char *who = "pdl_placement_batch_of_edges";
        if (n_queries == 0) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: no query", who);
        if (!out || !base || !n_query || !edge_begin) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: NULL pointer", who);
        for (uint32_t q = 0; q < n_queries; q++) {
            if (n_query[q] == 0) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: query %u: no query gene", who, q);
            if (edge_begin[q + 1] < edge_begin[q]) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: edge_begin decreases at query %u", who, q);
        }
        for (uint32_t q = 0; q < n_queries; q++)
            if (edge_begin[q + 1] - edge_begin[q] >= 0x7fffffffull || (uint64_t) base->sequences + n_query[q] >= 0x7fffffffull)
                PDL_FAIL(PDL_ERR_UNSUPPORTED, "%s: query %u: 2^31 genes or edges and more", who, q);
        // the lists as one upload: [edge_begin[0], edge_begin[n_queries]) of the caller's arrays, offsets from 0 from here on
        const uint64_t e0 = edge_begin[0], E = edge_begin[n_queries] - e0;
        check_base_pointers(who, base, genome_of, src, dst, E);
        std::vector<uint64_t> rel((size_t) n_queries + 1);
        for (uint32_t q = 0; q <= n_queries; q++) rel[q] = edge_begin[q] - e0;
        const PlaceBase B = upload_base(c, who, base, genome_of, src ? src + e0 : nullptr, dst ? dst + e0 : nullptr, E);
        std::vector<pdl_place_result> r;
        pdl_run_place_batch_edges(c, B, n_queries, n_query, rel.data(), c->pb.up_src.as<int32_t>(), c->pb.up_dst.as<int32_t>(), r);
        for (uint32_t q = 0; q < n_queries; q++) fill_placement(r[q], false, &out[q]);
        return PDL_OK;
    }, [&] { if (out) for (uint32_t q = 0; q < n_queries; q++) pdl_free_placement(&out[q]); });
}

int pdl_set_option(pdl_ctx *c, const char *name, int64_t value) {
    if (!c || !name) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, [&]() -> int {
    const std::string n(name);
    if (n == "join_tier1") {
        if (!(value == -1 || value == 0 || (value >= 9 && value <= 11) || value == 20 || value == 21)) PDL_FAIL(PDL_ERR_ARGUMENT, "join_tier1: -1, 0, 9, 10, 11, 20 or 21");
        c->opt_tier1 = (int) value;
    } else if (n == "join_tier0") c->opt_tier0 = value < 0 ? -1 : (value != 0);
    else if (n == "sift_threshold") {
        if (value != 0 && value != 1) PDL_FAIL(PDL_ERR_ARGUMENT, "sift_threshold: 0 or 1");
        c->opt_sift_threshold = (int) value;
    }
    else if (n == "join_tiny_tier2") c->opt_tiny_tier2 = value != 0;
    else if (n == "join_grid_pct") c->opt_grid_pct = (int) value;
    else if (n == "stage_timers") c->opt_stage_timers = value != 0;
    else if (n == "host_mirror") c->opt_host_mirror = value != 0;
    else if (n == "staging_cap") c->opt_staging_cap = value > 0 ? (uint64_t) value : 0;
    else if (n == "aside_test_reload") c->opt_aside_test_reload = value != 0;
    else if (n == "onepass_scan") c->opt_onepass_scan = value != 0;
    else if (n == "lean_radix") c->opt_lean_radix = value != 0;
    else if (n == "lean_records") c->opt_lean_records = value != 0;
    else if (n == "order_offsets") {
        if (value < 0 || value > 2) PDL_FAIL(PDL_ERR_ARGUMENT, "order_offsets: 0 (two scans), 1 (one workgroup) or 2 (several)");
        c->opt_order_offsets = (int) value;
    }
    else if (n == "order_offsets_rows") {
        if (value < 0) PDL_FAIL(PDL_ERR_ARGUMENT, "order_offsets_rows: a row count");
        c->opt_order_offsets_rows = (uint32_t) std::min<int64_t>(value, 0xffffffffll);
    }
    else if (n == "order_subwave") {
        if (!(value == 0 || value == 1 || value == 16 || value == 32)) PDL_FAIL(PDL_ERR_ARGUMENT, "order_subwave: 0 (a wave per row), 1 (the default width), 16 or 32 (lanes per row)");
        c->opt_order_subwave = (int) value;
    }
    else if (n == "order_wide_merged") {
        if (value != 0 && value != 1) PDL_FAIL(PDL_ERR_ARGUMENT, "order_wide_merged: 0 or 1");
        c->opt_order_wide_merged = value != 0;
    }
    else if (n == "fused_glue") {
        if (value < 0) PDL_FAIL(PDL_ERR_ARGUMENT, "fused_glue: 0, 1, or n > 1 (as 1, and K-len in one launch for up to n genes)");
        c->opt_fused_glue = (int) std::min<int64_t>(value, 0x7fffffff);
    }
    else if (n == "low_memory") c->opt_low_memory = value != 0;
    else if (n == "query_batch_bytes") {
        if (value <= 0) PDL_FAIL(PDL_ERR_ARGUMENT, "query_batch_bytes: a positive byte count");
        c->opt_query_batch_bytes = (uint64_t) value;
        return PDL_OK;        // (no bearing on a scoring pass: the context's scores stay)
    }
    else if (n == "split_scratch_bytes") {
        if (value <= 0) PDL_FAIL(PDL_ERR_ARGUMENT, "split_scratch_bytes: a positive byte count");
        c->opt_split_scratch_bytes = (uint64_t) value;
        return PDL_OK;        // (nor has this one)
    }
    else if (n == "matrix_slab_bytes") {
        if (value <= 0) PDL_FAIL(PDL_ERR_ARGUMENT, "matrix_slab_bytes: a positive byte count");
        c->opt_matrix_slab_bytes = (uint64_t) value;
        return PDL_OK;        // (nor has this one)
    }
    else if (n == "query_rekey") {
        if (value != 0 && value != 1) PDL_FAIL(PDL_ERR_ARGUMENT, "query_rekey: 0 or 1");
        c->opt_query_rekey = value != 0;
        return PDL_OK;        // (nor has this one)
    }
    else if (n == "alphabet_rekey") {
        if (value != 0 && value != 1) PDL_FAIL(PDL_ERR_ARGUMENT, "alphabet_rekey: 0 or 1");
        c->opt_alphabet_rekey = value != 0;
        return PDL_OK;        // (nor has this one)
    }
    else throw pdl_error{PDL_ERR_ARGUMENT, "unknown option " + n};
    pdl_stale(c, Stale::scores);        // the next scoring call runs with the new setting
    return PDL_OK;
    });
}

// ---- multi-GPU (see include/pandelos_amd.h) -------------------------------------------------------------------------
int pdl_dist_preprocess_begin(pdl_ctx *c, const uint8_t *d_residues, const uint64_t *d_offsets, const uint32_t *d_genome_of,
                              uint32_t n, uint64_t n_res, int k, uint32_t world, uint32_t rank, pdl_dist_slice *out) {
    if (!c || !out) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, [&]() -> int {
    if (!d_offsets || !d_genome_of || (!d_residues && n_res)) PDL_FAIL(PDL_ERR_ARGUMENT, "null input pointer");
    if (((uintptr_t) d_residues & 15) != 0) PDL_FAIL(PDL_ERR_ARGUMENT, "d_residues must be 16-byte aligned");
    if (world == 0 || rank >= world || world > 64) PDL_FAIL(PDL_ERR_ARGUMENT, "rank %u of %u (at most 64 ranks)", rank, world);
    PDL_HIP(hipSetDevice(c->device));
    pdl_stale(c, Stale::set);
    adopt_device_input(c, d_residues, d_offsets, d_genome_of, n, n_res);
    begin_build(c, n, n_res, k);
    build_genome_layout(c);
    c->world = world; c->rank = rank;
    c->shard.clear(); c->shard_set = false; c->dict_shard.clear();
    pdl_run_dist_begin(c, k);
    out->d_postings = c->post.p; out->records = c->U_slice; out->kmers = c->M_slice;
    out->genome_weights = c->h_run_weights.data(); out->genomes = c->G;
    out->genome_costs = c->h_run_costs.data();
    return PDL_OK;
    });
}

int pdl_dist_preprocess_finish(pdl_ctx *c, void *d_postings_all, uint64_t total_records, const uint64_t *genome_weights, pdl_cost *out_cost) {
    if (!c) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, [&]() -> int {
    require_state(c, E_DIST_FINISH);
    if (!d_postings_all || ((uintptr_t) d_postings_all & 7) != 0) PDL_FAIL(PDL_ERR_ARGUMENT, "the gathered dictionary must be an 8-byte aligned device array");
    if (total_records < c->U_slice) PDL_FAIL(PDL_ERR_ARGUMENT, "the gathered dictionary (%llu records) is smaller than this rank's run (%llu)",
                                             (unsigned long long) total_records, (unsigned long long) c->U_slice);
    PDL_HIP(hipSetDevice(c->device));
    c->post_ext = static_cast<uint2 *>(d_postings_all);
    pdl_run_dist_finish(c, total_records, genome_weights);
    c->preprocessed = true;
    fill_cost(c, out_cost);
    return PDL_OK;
    });
}

int pdl_dist_preprocess_ranges(pdl_ctx *c, const uint64_t *run_records, const uint64_t *genome_weights, const uint64_t *genome_costs, pdl_dist_ranges *out) {
    if (!c || !out || !run_records || !genome_weights || !genome_costs) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, [&]() -> int {
    require_state(c, E_DIST_RANGES);
    PDL_HIP(hipSetDevice(c->device));
    memset(out, 0, sizeof(*out));
    out->available = pdl_run_dist_ranges(c, run_records, genome_weights, genome_costs) ? 1 : 0;
    out->d_keys = c->dist_out_keys; out->d_ranges = reinterpret_cast<const uint64_t *>(c->dist_out_ranges);
    out->counts = c->h_tuple_counts.data(); out->total = c->dist_out_total;
    out->shared_records = c->dist_run_counters[0]; out->groups = c->dist_run_counters[1]; out->repeat_sample = c->dist_run_counters[2];
    return PDL_OK;
    });
}

int pdl_dist_preprocess_finish_ranges(pdl_ctx *c, void *d_postings_all, uint64_t total_records, uint32_t *d_keys, uint64_t *d_ranges, uint64_t n_tuples,
                                      const uint64_t *counter_sums, pdl_cost *out_cost) {
    if (!c || !counter_sums || ((!d_keys || !d_ranges) && n_tuples)) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, [&]() -> int {
    require_state(c, E_DIST_FINISH_RANGES);
    if (!d_postings_all || ((uintptr_t) d_postings_all & 7) != 0) PDL_FAIL(PDL_ERR_ARGUMENT, "the gathered dictionary must be an 8-byte aligned device array");
    if (n_tuples && ((((uintptr_t) d_keys) & 3) != 0 || (((uintptr_t) d_ranges) & 7) != 0)) PDL_FAIL(PDL_ERR_ARGUMENT, "the received tuples must be aligned device arrays");
    PDL_HIP(hipSetDevice(c->device));
    c->post_ext = static_cast<uint2 *>(d_postings_all);
    pdl_run_dist_finish_ranges(c, total_records, d_keys, reinterpret_cast<unsigned long long *>(d_ranges), n_tuples, counter_sums);
    c->preprocessed = true;
    fill_cost(c, out_cost);
    return PDL_OK;
    });
}

int pdl_dist_genome_owner(const pdl_ctx *cc, uint32_t *out) {
    pdl_ctx *c = const_cast<pdl_ctx *>(cc);
    if (!c || !out) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, [&]() -> int {
    require_state(c, E_DIST_GENOME_OWNER);
    memcpy(out, c->h_owner.data(), (size_t) c->G * 4);
    return PDL_OK;
    });
}

int pdl_dist_score_begin(pdl_ctx *c, pdl_dist_outbox *out) {
    if (!c || !out) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, [&]() -> int {
    require_state(c, E_DIST_SCORE_BEGIN);
    PDL_HIP(hipSetDevice(c->device));
    pdl_stale(c, Stale::scores);
    c->dist_stage = DistStage::adopted;
    pdl_run_dist_score_begin(c);
    out->d_cells = c->outbox.as<pdl_dist_cell>();
    out->counts = c->h_outbox_counts.data();
    out->total = 0;
    for (uint64_t v : c->h_outbox_counts) out->total += v;
    return PDL_OK;
    });
}

int pdl_dist_score_finish(pdl_ctx *c, const pdl_dist_cell *d_inbox, uint64_t n_inbox) {
    if (!c || (!d_inbox && n_inbox)) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, [&]() -> int {
    require_state(c, E_DIST_SCORE_FINISH);
    if (n_inbox >= 0xffffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "more than 2^32 received cells");
    PDL_HIP(hipSetDevice(c->device));
    pdl_run_dist_score_finish(c, d_inbox, n_inbox);
    return PDL_OK;
    });
}

int pdl_copy_device(pdl_ctx *c, void *d_dst, const void *d_src, uint64_t bytes) {
    if (!c || ((!d_dst || !d_src) && bytes)) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, [&]() -> int {
    PDL_HIP(hipSetDevice(c->device));
    if (bytes) PDL_HIP(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, c->stream));
    PDL_HIP(hipStreamSynchronize(c->stream));
    return PDL_OK;
    });
}

int pdl_get_dictionary(pdl_ctx *c, uint64_t *ranks, uint32_t *seqs, uint32_t *counts) {
    if (!c) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, [&]() -> int {
    require_state(c, E_GET_DICTIONARY);
    PDL_HIP(hipSetDevice(c->device));
    const uint64_t U = c->U, M = c->M;
    std::vector<uint32_t> recpos(U);
    std::vector<uint2> post(U);
    PDL_HIP(hipMemcpyAsync(recpos.data(), c->recpos.p, U * 4, hipMemcpyDeviceToHost, c->stream));
    PDL_HIP(hipMemcpyAsync(post.data(), c->post.p, U * 8, hipMemcpyDeviceToHost, c->stream));
    std::vector<uint8_t> keys(M * (c->key64 ? 8 : 4));
    PDL_HIP(hipMemcpyAsync(keys.data(), c->keys_b.p, keys.size(), hipMemcpyDeviceToHost, c->stream));
    PDL_HIP(hipStreamSynchronize(c->stream));
    for (uint64_t u = 0; u < U; u++) {
        if (ranks) ranks[u] = c->key64 ? reinterpret_cast<uint64_t *>(keys.data())[recpos[u]]
                                       : (uint64_t) reinterpret_cast<uint32_t *>(keys.data())[recpos[u]];
        if (seqs) seqs[u] = post[u].x;
        if (counts) counts[u] = post[u].y & 0x7fffffffu;       // (complexity-only mode leaves the group-head bit in place)
    }
    return PDL_OK;
    });
}

int pdl_query_scores(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, uint32_t n_query, pdl_scores *out, pdl_query_info *info) {
    if (!c) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    if (out) memset(out, 0, sizeof(*out));
    if (info) memset(info, 0, sizeof(*info));
    return guarded(c, [&]() -> int {
    require_state(c, E_QUERY_SCORES);
    if (!out) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_query_scores: NULL pointer");
    check_genes("pdl_query_scores", residues, offsets, n_query);
    PDL_HIP(hipSetDevice(c->device));
    query_rekey_open(c);
    pdl_run_query(c, residues, offsets, n_query, out, info);
    query_rekey_close(c);
    return PDL_OK;
    });
}

int pdl_query_batch(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, const uint32_t *gene_begin, uint32_t n, uint32_t n_queries,
                    pdl_scores *out, pdl_query_info *info, pdl_query_batch_info *binfo) {
    if (!c) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    if (out && n_queries) memset(out, 0, sizeof(*out) * (size_t) n_queries);
    if (info && n_queries) memset(info, 0, sizeof(*info) * (size_t) n_queries);
    if (binfo) memset(binfo, 0, sizeof(*binfo));
    return guarded(c, Lock::held, [&]() -> int {
        require_state(c, E_QUERY_BATCH);
        check_batch(c, "pdl_query_batch", out, residues, offsets, gene_begin, n, n_queries);
        PDL_HIP(hipSetDevice(c->device));
        query_rekey_open(c);
        pdl_run_query_batch(c, residues, offsets, gene_begin, n, n_queries, out, info, binfo);
        query_rekey_close(c);
        return PDL_OK;
    }, [&] {     // a refusal returns no block: what earlier chunks produced goes back, `out` is zero again
        if (out) for (uint32_t q = 0; q < n_queries; q++) pdl_free_scores(&out[q]);
        if (info && n_queries) memset(info, 0, sizeof(*info) * (size_t) n_queries);
        if (binfo) memset(binfo, 0, sizeof(*binfo));
    });
}

int pdl_append_genomes(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, const uint32_t *genome_of, uint32_t n, pdl_cost *out_cost,
                       pdl_append_info *info) {
    if (!c) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    if (info) memset(info, 0, sizeof(*info));
    return guarded(c, [&]() -> int {
    require_state(c, E_APPEND_GENOMES);
    check_genes("pdl_append_genomes", residues, offsets, n);
    // union genome ids: G, G+1, ... in first-seen order (PangeneIData.java:56-62 continued)
    std::vector<uint32_t> ids(n, c->G);
    uint32_t g_new = 1;
    if (genome_of) {
        g_new = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t g = genome_of[i];
            if (g < c->G) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_append_genomes: gene %u joins genome %u of the context (new genomes only: ids from %u)", i, g, c->G);
            if (g - c->G > g_new) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_append_genomes: genome id %u at gene %u is not dense in first-seen order (next new id: %u)", g, i, c->G + g_new);
            if (g - c->G == g_new) g_new++;
            ids[i] = g;
        }
    }
    PDL_HIP(hipSetDevice(c->device));
    pdl_run_append(c, residues, offsets, ids.data(), n, g_new, info);
    c->preprocessed = true;
    fill_cost(c, out_cost);
    return PDL_OK;
    });
}

int pdl_remove_genomes(pdl_ctx *c, const uint32_t *genomes, uint32_t count, pdl_cost *out_cost, pdl_remove_info *info) {
    if (!c) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    if (info) memset(info, 0, sizeof(*info));
    return guarded(c, [&]() -> int {
    require_state(c, E_REMOVE_GENOMES);
    if (!genomes) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_remove_genomes: NULL pointer");
    if (count == 0) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_remove_genomes: no genome");
    std::vector<uint8_t> named((size_t) c->G, 0);
    for (uint32_t i = 0; i < count; i++) {
        const uint32_t g = genomes[i];
        if (g >= c->G) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_remove_genomes: genome id %u out of range (%u genomes)", g, c->G);
        if (named[g]) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_remove_genomes: genome id %u is named twice", g);
        named[g] = 1;
    }
    if (count == c->G) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_remove_genomes: every genome of the context is named (nothing would remain)");
    PDL_HIP(hipSetDevice(c->device));
    pdl_run_remove(c, genomes, count, info);
    c->preprocessed = true;
    fill_cost(c, out_cost);
    return PDL_OK;
    });
}

int pdl_get_rekey_info(pdl_ctx *c, pdl_rekey_info *out) {
    if (!c || !out) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    *out = c->last_rekey;
    return PDL_OK;
}

int pdl_get_query_rekey_info(pdl_ctx *c, pdl_query_rekey_info *out) {
    if (!c || !out) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, [&]() -> int {
    *out = c->last_query_rekey;
    return PDL_OK;
    });
}

int pdl_get_query_join_info(pdl_ctx *c, pdl_query_join_info *out) {
    if (!c || !out) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, [&]() -> int {
    *out = c->last_query_join;
    return PDL_OK;
    });
}

int pdl_get_rank_table(const pdl_ctx *cc, uint8_t out[256], uint64_t *out_lm) {
    pdl_ctx *c = const_cast<pdl_ctx *>(cc);
    if (!c || !out) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, [&]() -> int {
    require_state(c, E_GET_RANK_TABLE);
    memcpy(out, c->rp.rank_values, 256);
    if (out_lm) *out_lm = c->rp.last_multiplier;
    return PDL_OK;
    });
}

int pdl_get_timings(pdl_ctx *c, pdl_timings *out) {
    if (!c || !out) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    *out = c->tm;
    return PDL_OK;
}

}  // extern "C"
