/*
 * pandelos_amd.h — C ABI of the MI355X-native PanDelos hot path
 * (k-mer dictionary matching + all-vs-all gene similarity scoring).
 *
 * This is the drop-in boundary.  In the reference the same boundary is the JNI pair
 *     Java_infoasys_cli_pangenes_PangeneNative_preprocessSequences   ig/native/pangene_native.h:16-17
 *     Java_infoasys_cli_pangenes_PangeneNative_computeScores         ig/native/pangene_native.h:24-25
 * implemented by ig/native/library.cpp:189-371 and :529-604 and declared on the Java side at
 * ig/infoasys/cli/pangenes/PangeneNative.java:14-15.  libnative.so (this project's JNI shim,
 * include/pdl_jni_abi.h + pandelos_amd/csrc/jni_shim.cpp) exports those two symbols and forwards
 * to the functions below; any other host (the Python mirror in pandelos_amd/, the C++ driver, a cgo /
 * N-API / ctypes stub) binds the functions below directly.
 *
 * Plain C: pointers and sizes only.  All work runs on one HIP device (gfx950); there is no CPU
 * fallback — pdl_create fails when no device is usable.
 */
#ifndef PANDELOS_AMD_H
#define PANDELOS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDL_API __attribute__((visibility("default")))

typedef struct pdl_ctx pdl_ctx;

enum {
    PDL_OK = 0,
    PDL_ERR_KVALUE = -1,       /* k <= 0: the reference prints "K value must be greater than 0." and exit(1)s (library.cpp:90-93) */
    PDL_ERR_EMPTY = -2,        /* no k-mer at all: undefined behaviour in the reference (library.cpp:297) */
    PDL_ERR_ARGUMENT = -3,     /* NULL pointer, genome id out of range, ... */
    PDL_ERR_DEVICE = -4,       /* a HIP call failed; see pdl_last_error */
    PDL_ERR_STATE = -5,        /* compute before preprocess, etc. */
    PDL_ERR_UNSUPPORTED = -6   /* input outside the implemented domain (stated in the message) */
};

typedef struct {
    int32_t device;            /* HIP device ordinal; -1 = current device */
    void *stream;              /* hipStream_t to run on; NULL = a stream owned by the context */
    uint32_t flags;            /* PDL_FLAG_* */
    uint32_t reserved;
} pdl_config;

#define PDL_FLAG_CANONICAL_ORDER 1u  /* emit each row's cells by ascending column instead of the reference's
                                        first-touch order (library.cpp:456-482,493); cheaper, same cell set */

/* What preprocessSequences prints as its cost model (library.cpp:337-350) plus the sizes every
 * run must report for the roofline (R, M, U, P). */
typedef struct {
    uint64_t residues;          /* R */
    uint64_t kmer_occurrences;  /* M  = sum over genes of max(len-k+1, 0) */
    uint64_t dictionary_records;/* U  = unique (rank, gene) records (library.cpp:280-287) */
    uint64_t shared_records;    /* U' = records in rank-groups with >= 2 records (= posting ranges, library.cpp:318-326) */
    uint64_t groups;            /* rank-groups with >= 2 records (multi-GPU: counted over the whole dictionary as well) */
    uint64_t total_cost;        /* P  = "Total cost: P lookups" (library.cpp:327,349) */
    float linear_ratio;         /* P / sum kseq_lengths (library.cpp:350) */
    uint32_t sequences;         /* N */
    uint32_t genomes;           /* G */
    uint32_t rank_base;         /* alphabet size B (library.cpp:96-100) */
    uint32_t rank_bits;         /* bits needed for a rank (64 in hash mode) */
    int32_t hash_fallback;      /* 1 when B^k overflows 64 bits (library.cpp:103-119) */
    int32_t kvalue;
} pdl_cost;

/* Flat mirror of ig/infoasys/cli/pangenes/Scores.java:4-34 exactly as library.cpp:542-603 fills it.
 * All arrays are host memory owned by the library until pdl_free_scores. */
typedef struct {
    uint32_t scoresCount;
    uint32_t rows;                 /* genes of this genome = first dimension of max_genome_score */
    uint32_t genomes;              /* G = second dimension of max_genome_score */
    uint32_t sequences;            /* N = length of max_genome_score_col and scoresMaxMappings */
    float *scores;                 /* [scoresCount] */
    float *percs;                  /* [scoresCount] */
    float *tr_percs;               /* [scoresCount] */
    int32_t *row;                  /* [scoresCount] */
    int32_t *column;               /* [scoresCount] */
    int32_t *first_seq_genome;     /* [scoresCount] */
    int32_t *second_seq_genome;    /* [scoresCount] */
    float *max_genome_score;       /* [rows][genomes] row-major (Java float[][]) */
    float *max_genome_score_col;   /* [sequences] */
    int32_t *scoresMaxMappings;    /* [sequences]; INT32_MAX for genes of other genomes (library.cpp:428-432) */
} pdl_scores;

/* Device time of the stages of the last preprocess / score pass, from HIP events on the context's
 * stream (milliseconds), and the counters the roofline needs. */
typedef struct {
    float hist_ms, rank_ms, sort_rank_ms, dict_ms, sort_seq_ms, ranges_ms;  /* preprocess */
    float join_ms, join_overflow_ms, order_ms;                             /* scoring: the join's three tiers; of which the HBM-table tier; K-order */
    float preprocess_total_ms, score_total_ms;
    uint64_t emitted_cells;        /* Z over the genomes scored by this context */
    uint64_t scored_rows;          /* rows (genes) scored by this context */
    uint64_t scored_lookups;       /* P restricted to those rows */
    uint64_t overflow_rows;        /* rows that left the LDS tables for the HBM table (tier 3) */
    uint32_t join_launches;
    uint32_t tier2_rows;           /* rows the filtered small-table tier handed to the big LDS table */
    /* multi-GPU passes (zero otherwise) */
    float dist_begin_ms, dist_finish_ms;   /* pdl_dist_preprocess_begin / _finish, device time */
    float dist_score_begin_ms, dist_score_finish_ms;
    uint64_t walked_lookups;       /* postings the join actually read: each unordered pair of a group once when rows only meet the genes above them */
    uint64_t outbox_cells, inbox_cells;
    uint64_t aside_reloads;        /* join, filter tier: entries of a put-aside list that did not yet show what the wave had stored there
                                      when it first read them back (they are loaded again until they do) */
    uint32_t aside_repeats;        /* scoring passes thrown away and repeated with fully tagged (16-byte) list entries because a pass with
                                      the 10-bit tags saw a reload: no result is ever returned from such a pass */
    uint32_t tier1_rows;           /* rows that reached the filtered small-table tier (all of them unless the partition tier ran in front) */
    float reshard_ms;              /* the range lists built again for another genome shard on the existing dictionary (pdl_set_genome_shard after pdl_preprocess) */
    float dist_ranges_ms;          /* pdl_dist_preprocess_ranges, device time (0 when the owners build the range lists) */
} pdl_timings;

PDL_API pdl_ctx *pdl_create(const pdl_config *cfg /* may be NULL */);
PDL_API void pdl_destroy(pdl_ctx *);
/* Message of the last failure on this context (or of pdl_create when ctx == NULL); never NULL. */
PDL_API const char *pdl_last_error(const pdl_ctx *);

/* preprocessSequences (library.cpp:189-371).  Gene i is residues[offsets[i] .. offsets[i+1]), one byte
 * per character (the reference reads UTF-16 units and is only defined for units < 256, library.cpp:76,223);
 * genome_of[i] is its dense genome id in first-seen order (PangeneIData.java:56-62).  Resets the context
 * (library.cpp:192).  only_complexity != 0 stops after the cost model (PangeneNative.java:10-12).
 * The _host form takes host pointers and copies them to the device; the _device form takes device
 * pointers that must stay valid until the next preprocess or destroy. */
PDL_API int pdl_preprocess(pdl_ctx *, const uint8_t *residues, const uint64_t *offsets,
                           const uint32_t *genome_of, uint32_t n_sequences, int kvalue,
                           int only_complexity, pdl_cost *out_cost /* may be NULL */);
PDL_API int pdl_preprocess_device(pdl_ctx *, const uint8_t *d_residues, const uint64_t *d_offsets,
                                  const uint32_t *d_genome_of, uint32_t n_sequences, uint64_t n_residues,
                                  int kvalue, int only_complexity, pdl_cost *out_cost);

/* ---- ingest: .faa -> HBM (the Java side's PangeneIData.readFromFile, PangeneIData.java:30-75, and calculate_k.py:9-30) --
 * One pass over the mapped file: readLine's terminators (\n, \r, \r\n), String.trim, blank lines skipped, header / sequence
 * alternating, genome = the header's text before the first tab, ids dense in first-seen order; a header with fewer than three
 * tab-separated fields fails (the reader indexes cc[1], cc[2]).  Sequence bytes are copied once, into pinned staging buffers
 * that leave for the device while the parser goes on.  k_suggested is what calculate_k.py prints for the same file (raw line
 * parity, str.strip, entropy summed in first-seen letter order; 0 where the script would divide by zero). */
typedef struct {
    uint64_t file_bytes;
    uint64_t residues;             /* R */
    uint32_t sequences, genomes;   /* N, G */
    int32_t k_suggested;
    uint32_t reserved;
    double parse_ms;               /* wall time: open -> last byte on the device (pdl_scan_faa: -> parsed) */
    const uint64_t *offsets;       /* host [sequences + 1], owned by the context until its next ingest (pdl_scan_faa: NULL) */
    const uint32_t *genome_of;     /* host [sequences] */
    const uint8_t *d_residues;     /* device, owned by the context: the arguments of pdl_preprocess_device / pdl_dist_preprocess_begin */
    const uint64_t *d_offsets;
    const uint32_t *d_genome_of;
} pdl_ingest;
PDL_API int pdl_ingest_faa(pdl_ctx *, const char *path, pdl_ingest *out);
/* genome names in id order (PangeneIData.genomeNames); NULL when out of range */
PDL_API const char *pdl_ingest_genome_name(const pdl_ctx *, uint32_t genome);
/* preprocessSequences on the ingested input (no copy, no read-back of the genome ids) */
PDL_API int pdl_preprocess_ingested(pdl_ctx *, int kvalue, int only_complexity, pdl_cost *out_cost /* may be NULL */);
/* The same parser without a device or a context, into caller buffers (each may be NULL: count only).  Errors: pdl_last_error(NULL). */
PDL_API int pdl_scan_faa(const char *path, pdl_ingest *out, uint8_t *residues, uint64_t cap_residues, uint64_t *offsets /* [cap_sequences + 1] */,
                         uint32_t *genome_of, uint32_t cap_sequences);

/* "Genome g cost = ..." (library.cpp:535-538) */
PDL_API int pdl_genome_cost(const pdl_ctx *, uint32_t genome, uint64_t *out_cost);
/* Per-gene cost (computation_costs[].total_visited, library.cpp:327) and k-mer count (kseq_lengths, :250-262) */
PDL_API int pdl_sequence_costs(const pdl_ctx *, uint64_t *out_total_visited /* [N] */, uint32_t *out_kseq_lengths /* [N], may be NULL */);

/* Restrict the genomes this context scores (multi-GPU sharding: one context per GPU, each with the
 * full dictionary postings and a disjoint genome list).  Must be set BEFORE pdl_preprocess: the
 * posting-range lists, per-gene costs and pdl_cost.total_cost are then built for the shard's genes only
 * (the part of the dictionary build that is proportional to the rows scored).  Without a shard the
 * range lists hold only the genes above each row and every cell is produced once for both of its rows, so
 * a dictionary built for all genomes cannot score a subset (PDL_ERR_STATE).  A dictionary built for a shard can be
 * narrowed further — or pointed at ANOTHER shard: the postings stay, the range lists of the new shard's genes are built
 * before the next scoring pass (two passes over the postings; pdl_timings.reshard_ms).  That is how a set too large for one
 * device's memory is scored a batch of genomes at a time (the reference's unit of work, Pangenes.java:60-66, with the
 * reference's per-task scratch, library.cpp:417-428): shard = batch 0, pdl_preprocess, fetch the batch's Scores, shard =
 * batch 1, fetch, ... — only one batch's maxima, staging and cells are on the device at a time (option "low_memory" also
 * returns the build's transient buffers).  count == 0 clears the shard.  The shard stays in force across pdl_preprocess calls. */
PDL_API int pdl_set_genome_shard(pdl_ctx *, const uint32_t *genomes, uint32_t count);

/* computeScores for every genome of the shard in one device pass (library.cpp:409-527 for each
 * genome); results stay in HBM.  Idempotent until the next preprocess. */
PDL_API int pdl_score_all(pdl_ctx *);

/* computeScores + the marshalling of library.cpp:542-603 for one genome: runs pdl_score_all on first
 * use, then copies that genome's block to the host.  Re-entrant from several host threads, like the
 * reference (Pangenes.java:54-66). */
PDL_API int pdl_compute_scores(pdl_ctx *, uint32_t genome, pdl_scores *out);
PDL_API void pdl_free_scores(pdl_scores *);

/* The host stage behind computeScores, on the device: the bidirectional-best-hit filter of Pangenes.java:98-176 over one
 * genome task's cells.  Returns the edges that task adds to the network in the host's insertion order — phase 1 (inter-genome
 * best hits, (row, column) then (column, row) per cell), then phase 2 (kept intra-genome cells) — i.e. exactly the
 * addConnection calls of Pangenes.java:103-104,171-175; what is left to the host is the network container and its
 * text form (PangeneNet.java).  The first call filters every genome of the context and brings all edges to the host once. */
typedef struct {
    uint32_t count;
    int32_t *src, *dst;            /* [count] gene ids */
    float *score;                  /* [count] */
} pdl_edges;
PDL_API int pdl_compute_edges(pdl_ctx *, uint32_t genome, pdl_edges *out);
PDL_API void pdl_free_edges(pdl_edges *);

/* ---- query: one new genome against the dictionary already built (no rebuild) --------------------------------------
 * Returns the block computeScores(G) (library.cpp:409-527, marshalled as :542-603) returns for the UNION run: the base genes
 * 0..N-1 in base order, then the n_query genes of residues/offsets as genome G (ids N..N+n_query-1), same k.  rows = n_query,
 * genomes = G+1, sequences = N+n_query; first_seq_genome == G for every cell; PDL_FLAG_CANONICAL_ORDER orders each row by
 * column.  Only that task's block: the other genomes' maxima would change in a full run and are not produced.  The base
 * context is left as it was (scores, edges, dictionary, costs, timings); queries are independent of each other; the query's
 * buffers are reused and released at the next preprocess or destroy.  Free `out` with pdl_free_scores.
 * PDL_ERR_STATE: no preprocess, only_complexity, a multi-GPU context, or low_memory released the sorted k-mer stream.
 * PDL_ERR_ARGUMENT: n_query == 0, NULL pointers, decreasing offsets.  PDL_ERR_UNSUPPORTED: a query byte the base's alphabet
 * lacks (the union would have another rank table, library.cpp:96-119; the message names the byte) unless option "query_rekey"
 * is on (see there: the query is then ranked in the union's alphabet), genes of 2^20 k-mers or more, or union sizes past the
 * base build's limits (2^32 residues, 31-bit gene ids). */
typedef struct {
    uint64_t residues, kmer_occurrences;   /* of the query */
    uint64_t records;          /* unique (rank, query gene) records */
    uint64_t matched_records;  /* query records whose k-mer (rank) the base dictionary holds; a record whose union group gains a
                                  base record only through the union's last-record fold does not count: that record's k-mer differs */
    uint64_t genome_cost;      /* "Genome G cost" of the union run (library.cpp:327,535-538) */
    float device_ms;           /* device time of the call: the sum of its stretches of device work (HIP event pairs), without the
                                  host's reads in between (the record count and staging bound; whether a row left the LDS table) */
} pdl_query_info;
PDL_API int pdl_query_scores(pdl_ctx *, const uint8_t *residues, const uint64_t *offsets /* [n_query+1] */,
                             uint32_t n_query, pdl_scores *out, pdl_query_info *info /* may be NULL */);

/* pdl_get_query_join_info: which way the rows of the last successful pdl_query_scores, pdl_query_batch, pdl_place_query or
 * pdl_place_batch took through the query's join (all of a batch's chunks together).  A query gene is one row: one workgroup on a
 * table in LDS, and, when its columns do not fit that table, one of at most 16 workgroups on dense tables in HBM that the context
 * keeps between calls.  Everything here is what the host already held when the call returned; a refused call leaves the report
 * of the last successful one. */
typedef struct {
    uint64_t rows;              /* query genes handed to the join (none for a query or chunk without a k-mer) */
    uint64_t may_overflow_rows; /* rows with more lookups than the LDS table takes keys: the host then looks whether one left it */
    uint64_t overflow_rows;     /* rows that did leave the LDS table and ran on the tables in HBM */
    uint32_t hbm_launches;      /* launches of the HBM kernel (one per query or chunk with such a row) */
    uint32_t hbm_workgroups;    /* the most workgroups one of them had */
    uint32_t hbm_clears;        /* launches for which the tables were allocated or cleared rather than taken as they were */
} pdl_query_join_info;
PDL_API int pdl_get_query_join_info(pdl_ctx *, pdl_query_join_info *out);

/* ---- query batch: q new genomes against the dictionary already built, each on its own, in one pass -------------------
 * The n genes of residues/offsets are cut into n_queries genomes by gene_begin: the genes of query j are
 * [gene_begin[j], gene_begin[j+1]).  out[j] is, bit for bit and in emission order, the block pdl_query_scores returns for the
 * genes of query j alone on this context: computeScores(G) of the union of the base and genome j only — its genes are ids
 * N..N+n_j-1 of genome G in its own block, sequences = N+n_j, genomes = G+1; PDL_FLAG_CANONICAL_ORDER is honoured.  The queries
 * never see each other (that is an append) and the base context is only read.  info[j] holds query j's own sizes, matched
 * records and "Genome G cost"; its device_ms is an even share of its chunk's device time.  The stages run once over all genes
 * of a chunk of consecutive queries; a chunk holds as many queries as option "query_batch_bytes" allows (at least one), the
 * results do not depend on the chunking.  Free every out[j] with pdl_free_scores.
 * Every refusal is decided before a block is returned: `out` is left zeroed and the context as it was.
 * PDL_ERR_STATE: as pdl_query_scores.  PDL_ERR_ARGUMENT: n_queries == 0, n == 0, NULL pointers, decreasing offsets, a gene_begin
 * that does not start at 0, does not end at n or is not strictly increasing (a query without genes).  PDL_ERR_UNSUPPORTED: a
 * byte the base's alphabet lacks (the message names the first such query and its smallest absent byte; with option "query_rekey"
 * only a query whose own union has no exact ranks is refused so), a gene of 2^20 k-mers
 * or more, a batch whose residues pass 2^32 with the base's, or N + n_j past the 31-bit gene ids (decided from gene_begin alone,
 * before offsets is read). */
typedef struct {
    uint32_t queries, chunks;  /* queries scored; chunks of consecutive queries the call worked through */
    float device_ms;           /* device time of the call, as pdl_query_info.device_ms, over all chunks */
} pdl_query_batch_info;
PDL_API int pdl_query_batch(pdl_ctx *, const uint8_t *residues, const uint64_t *offsets /* [n+1] */,
                            const uint32_t *gene_begin /* [n_queries+1]: genes of query j = [gene_begin[j], gene_begin[j+1]) */,
                            uint32_t n, uint32_t n_queries,
                            pdl_scores *out /* [n_queries], each freed with pdl_free_scores */,
                            pdl_query_info *info /* [n_queries] or NULL */,
                            pdl_query_batch_info *binfo /* may be NULL */);

/* ---- append: new genomes join the dictionary already built, by a merge instead of a rebuild ----------------------------
 * The n genes of residues/offsets become genes N..N+n-1 of the context.  genome_of == NULL: all of them are ONE new genome G.
 * Otherwise genome_of[i] are union ids G..G+g-1, dense in first-seen order (the rule of PangeneIData.java:56-62 continued); an id
 * below G (a gene added to an existing genome) or one that skips an id is PDL_ERR_ARGUMENT.
 * After PDL_OK every observable of the context equals, bit for bit, that of a context on which pdl_preprocess ran with the union
 * (base genes first, same k, same flags and options): pdl_cost, pdl_get_dictionary, pdl_genome_cost, pdl_sequence_costs,
 * pdl_get_rank_table, pdl_compute_scores / pdl_score_all / pdl_scores_counts for all G+g genomes, pdl_compute_edges, and later
 * pdl_query_scores and later appends.  Scores, edges and query buffers of the old context are dropped (as by a preprocess).
 * pdl_get_timings: the preprocess stage fields describe the append — rank_ms: K-rank of the new genes; sort_rank_ms: their sort
 * plus the merge pass; dict_ms, sort_seq_ms, ranges_ms: the stages behind the sorted stream, which run over the whole union;
 * hist_ms 0; preprocess_total_ms = pdl_append_info.device_ms — and the scoring fields start again at zero.
 * The base's residues are not needed and not touched: the call works after pdl_preprocess, pdl_preprocess_device (the caller's
 * input buffers may be gone: from here on the context owns its copy of the genome ids) and pdl_preprocess_ingested.  The sorted
 * k-mer stream of the union is the stable merge of the base's (in HBM) and the new genes' (K-rank + K-sort with the base's rank
 * table): one pass over it, then the stages behind the sort as in a build.
 * Refusals, checked BEFORE anything is changed (the context stays exactly as it was: scores, edges, dictionary, costs, timings):
 * PDL_ERR_STATE before a preprocess, after only_complexity, on a multi-GPU context, with a genome shard in force, or after
 * low_memory released the sorted k-mer stream; PDL_ERR_ARGUMENT for n == 0, NULL pointers, decreasing offsets, bad genome_of;
 * PDL_ERR_UNSUPPORTED for a byte the base's alphabet lacks (the union would have another rank table, library.cpp:96-119; the
 * message names the byte) and for unions past the build's limits (2^32 residues / k-mer positions, 31-bit gene ids).  Appended
 * genes with no k-mer at all (shorter than k, empty) are legal: they become genes with kseq_len 0.
 * A device failure in the middle (PDL_ERR_DEVICE) leaves the context un-preprocessed: PDL_ERR_STATE until the next pdl_preprocess. */
typedef struct {
    uint64_t residues, kmer_occurrences;   /* of the appended genes */
    uint64_t records;                      /* their unique (rank, gene) records */
    float rank_sort_ms;                    /* K-rank + K-sort of the appended genes (0 with option "stage_timers" 0, like merge_ms) */
    float merge_ms;                        /* the merge pass */
    float device_ms;                       /* the whole call on the device (the sum of its stretches of device work) */
} pdl_append_info;
PDL_API int pdl_append_genomes(pdl_ctx *, const uint8_t *residues, const uint64_t *offsets /* [n+1] */,
                               const uint32_t *genome_of /* [n] or NULL */, uint32_t n,
                               pdl_cost *out_cost /* may be NULL: the union's */, pdl_append_info *info /* may be NULL */);

/* ---- remove: genomes leave the dictionary already built, by a compaction instead of a rebuild --------------------------
 * The genes of the `count` listed genomes leave the context.  After PDL_OK every observable of the context equals, bit for bit,
 * that of a context on which pdl_preprocess ran with the REMAINING SET: the remaining genes in their input order with ids dense
 * from 0, the remaining genomes with ids dense in first-seen order (the order they have, closed up), same k, flags and options:
 * pdl_cost (residues included), pdl_get_dictionary, pdl_get_rank_table, pdl_genome_cost, pdl_sequence_costs, pdl_compute_scores /
 * pdl_score_all / pdl_scores_counts, pdl_compute_edges, pdl_compute_families, and later queries, appends and removals.  Scores,
 * edges, families and query buffers of the old context are dropped, as by an append.  Genomes may be interleaved gene by gene,
 * may be the first, a middle or the last one, and several may go in one call; replace = remove + append, append + remove undoes.
 * pdl_get_timings: the preprocess stage fields describe the removal — hist_ms and rank_ms 0; sort_rank_ms: the compaction pass over
 * the sorted k-mer stream (with the gene map and the alphabet check); dict_ms, sort_seq_ms, ranges_ms: the stages behind the sorted
 * stream, over what remains; preprocess_total_ms = pdl_remove_info.device_ms — and the scoring fields start again at zero.
 * No residue is needed: the sorted k-mer stream in HBM, sorted by (rank, input position), loses the k-mers of the leaving genes
 * in one stable pass and the gene ids are renumbered monotonically — the stream pdl_preprocess would sort for the remaining set,
 * PROVIDED the rank table is the same.
 * Refusals, checked BEFORE anything is changed (the context stays exactly as it was: scores, edges, dictionary, costs, timings):
 * PDL_ERR_STATE before a preprocess, after only_complexity, on a multi-GPU context, with a genome shard in force, or after
 * low_memory released the sorted k-mer stream; PDL_ERR_ARGUMENT for a NULL list, count == 0, an id >= G, an id named twice, every
 * genome named; PDL_ERR_EMPTY when the remaining genes hold no k-mer (what pdl_preprocess answers for such a set);
 * PDL_ERR_UNSUPPORTED when the remaining set cannot be shown to have the context's alphabet — if every occurrence of a letter
 * leaves, the remaining set's rank table differs (library.cpp:96-119).  The proof comes from the keys in HBM: polynomial ranks with
 * an exact B^k are sum v[c_i] * B^(k-1-i) with dense digits v, so the digits of the keys that stay name letters that are certainly
 * present; all B of them must show.  A letter that survives only in genes shorter than k is not seen: the refusal is conservative
 * in that one direction, and the message says so and names the smallest letter not found.  Hashed ranks (hash_fallback) and ranks
 * that wrapped past 2^64 (22 letters at k = 15 and the like) cannot be decoded and are refused with their own message.  After
 * PDL_ERR_UNSUPPORTED the caller rebuilds from the remaining genes.
 * A device failure in the middle (PDL_ERR_DEVICE) leaves the context un-preprocessed: PDL_ERR_STATE until the next pdl_preprocess. */
typedef struct {
    uint64_t sequences;                    /* genes that left */
    uint64_t residues, kmer_occurrences;   /* of those genes */
    uint64_t records;                      /* their unique (rank, gene) records */
    float compact_ms;                      /* gene map + compaction pass + alphabet check: the call's first stretch of device work */
    float device_ms;                       /* the whole call on the device (the sum of its stretches of device work, as pdl_append_info) */
} pdl_remove_info;
PDL_API int pdl_remove_genomes(pdl_ctx *, const uint32_t *genomes /* [count] distinct ids < G */, uint32_t count,
                               pdl_cost *out_cost /* may be NULL: the remaining set's */, pdl_remove_info *info /* may be NULL */);

/* ---- append and remove across a change of the alphabet: option "alphabet_rekey" ------------------------------------------
 * With the option at 0 (the default) both calls above refuse whatever changes the alphabet, as described.  With it at 1:
 *   pdl_append_genomes accepts bytes the base lacks.  The union's rank table is made on the host from the base's letters and the
 *     new genes' (all of them, genes shorter than k included, as a build counts them); the base's sorted stream is written again,
 *     key by key, in the union's base with the union's digits (one streaming pass, no sort: adding letters moves digits
 *     monotonically, so order and equality of keys are kept); the new genes are ranked with the union's table and merged in.
 *   pdl_remove_genomes is exact in both directions, provided the context was BUILT with the option on: pdl_preprocess (all three
 *     forms) then records, per genome, the letters of its genes shorter than k — the ones no key shows — in a table the context owns
 *     and appends and removals keep up.  The remaining alphabet is the digits of the keys that stay plus those letters of the genomes
 *     that stay.  Equal to the context's: the removal goes through (also where the default refuses conservatively).  Smaller: the
 *     compacted stream is written again for the smaller alphabet.  Without the table (the option was set after the build) a removal
 *     that misses a digit is refused as by default, and the message names the option; an append does not need the table.
 * The key width follows the new table in both directions (ACGT at k = 16 has 32-bit keys, ACGTN 38-bit ones).
 * Both need ranks that are the polynomial itself BEFORE and AFTER the call: no hash fallback, B^k < 2^64.  Otherwise
 * PDL_ERR_UNSUPPORTED, and the message says which side is hashed or wrapped; like every refusal it comes before anything changes.
 * After PDL_OK the context equals, bit for bit, what pdl_preprocess leaves on the union / the remaining set: the contract above.
 * pdl_get_timings: the re-key pass counts into sort_rank_ms (with "stage_timers" 0 it is not timed apart and shows only in the totals).
 * Queries and placements with a byte the base lacks keep refusing under this option; option "query_rekey" below is theirs.
 * pdl_get_rekey_info: what the last successful pdl_append_genomes / pdl_remove_genomes of the context did about the alphabet. */
typedef struct {
    uint32_t letters_before, letters_after;     /* B of the rank table before and after the call */
    uint32_t key_bits_before, key_bits_after;   /* rank_bits: 32-bit keys up to 32, 64-bit keys above */
    uint64_t keys_rewritten;                    /* elements of the sorted stream written again (0: no re-key) */
    float rekey_ms;                             /* the re-key pass on the device (0 with option "stage_timers" 0) */
    uint32_t rekeyed;                           /* 1: the call changed the rank table */
} pdl_rekey_info;
PDL_API int pdl_get_rekey_info(pdl_ctx *, pdl_rekey_info *out);

/* ---- query and place a genome that brings letters the base lacks: option "query_rekey" --------------------------------------
 * With the option at 0 (the default) pdl_query_scores, pdl_query_batch, pdl_place_query and pdl_place_batch refuse a query byte
 * the base's alphabet lacks, as described with each.  With it at 1 they accept such bytes:
 *   The union's rank table is made on the host from the base's letters and ALL the query's (genes shorter than k included, as a
 *     build counts them).  The query is ranked with it; its records are then written back, digit by digit, into the base's
 *     alphabet to search the base's keys, which are not touched: the digit map between an alphabet and a superset of it is
 *     strictly increasing, so order and equality of k-mers are the same on both sides, and a k-mer with a new letter equals no
 *     base k-mer.  The key width follows the union (ACGT at k = 16 has 32-bit keys, with N the query's are 38-bit ones).
 *   pdl_query_scores: the block, pdl_query_info.genome_cost, records and matched_records are what the reference returns for task
 *     G of the union run, bit for bit and in emission order.
 *   pdl_query_batch: block j is what pdl_query_scores returns for query j alone, whatever letters the other queries bring and
 *     however the batch is chunked.  A chunk is ranked once, with the letters of all its queries — a block is the same in whichever
 *     exact superset alphabet it was ranked — and is cut in front of the query that would make that alphabet inexact.
 *   pdl_place_query, pdl_place_batch: the query's edges and every placement field follow from that block as before.
 * The base context is only read: scores, edges, families, dictionary, costs, timings, the rank table and pdl_get_rekey_info are the
 * same before and after, and a later query without a new letter behaves exactly as with the option off.
 * Both sides need ranks that are the polynomial itself: PDL_ERR_UNSUPPORTED when the base's ranks are hashed or wrapped past 2^64,
 * or those of the union of the base and THIS query alone would be; the message names the byte, says which side, and names the
 * option.  In a batch the verdict is each query's own, and the message names the first refused query.  Every other refusal of the
 * four keeps its code and words, and like them these come before a block is returned and leave the context as it was.
 * pdl_get_query_rekey_info: what the last successful call of the four did about letters (all of a batch's chunks together). */
typedef struct {
    uint32_t queries_rekeyed;                   /* queries that brought a letter the base lacks */
    uint32_t letters_base;                      /* B of the base's rank table */
    uint32_t letters_max;                       /* the most letters a query's own union had (letters_base: no query brought one) */
    uint32_t key_bits_base;                     /* rank_bits of the base: 32-bit keys up to 32, 64-bit keys above */
    uint32_t key_bits_max;                      /* the widest rank_bits a query or a chunk was ranked with */
    uint64_t records_rebased;                   /* query records written back into the base's alphabet */
    float rebase_ms;                            /* that pass on the device (0 with option "stage_timers" 0) */
} pdl_query_rekey_info;
PDL_API int pdl_get_query_rekey_info(pdl_ctx *, pdl_query_rekey_info *out);

/* ---- gene families: the network's components and their collisions, on the device, from the edges where they lie --------
 * What netclu_ng.py does with the .net before Girvan-Newman: the connected components of the gene network (:58-66) and, per
 * component, whether it holds a collision — two genes of one genome that are not adjacent (get_max_collision, :75-92).  A
 * component without one is a gene family as it stands; only the colliding ones need the host's split
 * (pandelos_amd/netclu.py, families_from_components).  Edges are read as netclu_ng.py:41-56 reads them: undirected, a repeated
 * pair is one edge, a self edge makes its gene a node but is no edge.
 * pdl_compute_families: over the context's own edges — runs the scoring pass and the best-hit filter on first use, like
 * pdl_compute_edges, then K-fam over the edges in HBM (no edge crosses PCIe for it).  Cached until the next preprocess, append
 * or scoring pass; scores, edges, dictionary, costs and pdl_timings are left as they were; after pdl_append_genomes it answers
 * for the union.  PDL_ERR_STATE before a preprocess, after only_complexity, on a multi-GPU context, and with a genome shard in
 * force (genome batches, option "low_memory"): the context then does not hold every genome's edges — gather them and use
 * pdl_families_of_edges: the same kernels over a caller's edge list (host pointers; of the context only the device, the stream
 * and work buffers are used, no preprocess is needed and the context's own state is not changed).  PDL_ERR_ARGUMENT: NULL
 * pointers, a gene id that is negative or >= n_sequences (counted on the device BEFORE anything is indexed by an id; an error
 * return, nothing more).  n_edges == 0 is legal: nodes = families = 0.  Free with pdl_free_families. */
typedef struct {
    uint32_t sequences;       /* N */
    uint32_t nodes;           /* genes with at least one edge (self edges count): len(adj) of netclu.read_net */
    uint32_t families;        /* F: connected components of the network */
    uint32_t colliding;       /* components that hold a collision (netclu_ng.py:75-92) */
    uint32_t *component_of;   /* [N] smallest gene id of the gene's component; its own id for a gene that is no node */
    uint8_t  *is_node;        /* [N] */
    uint32_t *family_off;     /* [F+1] into family_genes; families in ascending order of their label */
    uint32_t *family_genes;   /* [nodes] ascending gene ids inside a family */
    uint8_t  *collides;       /* [F] */
    float device_ms;          /* sum of the stretches of device work (HIP event pairs: the id check of a caller's list, then
                                 everything up to the read of the counts), as pdl_query_info.device_ms; uploads and the copies
                                 of the arrays to the host are not in it */
} pdl_families;
PDL_API int pdl_compute_families(pdl_ctx *, pdl_families *out);
PDL_API int pdl_families_of_edges(pdl_ctx *, const int32_t *src, const int32_t *dst, uint64_t n_edges,
                                  const uint32_t *genome_of /* [n_sequences] */, uint32_t n_sequences, pdl_families *out);
PDL_API void pdl_free_families(pdl_families *);

/* ---- split: the first level of Girvan-Newman on a batch of ordered graphs, on the device -----------------------------------
 * What netclu.girvan_newman_first_level does to a component that holds a collision (netclu_ng.py:97-111 through networkx): the
 * edge of highest UNWEIGHTED shortest-path betweenness is removed, the betweenness of the whole graph is computed again, and so
 * on until the removed edge's two ends are no longer connected (the component count has grown).  The orders that decide ties
 * stay with the caller: graph j is the ordered adjacency g = rebuilt(rebuilt(view)), flattened — local node i is the i-th key of
 * g, adj[adj_off[node] .. adj_off[node + 1]) its neighbours in dict order as LOCAL indices (node = node_off[j] + i; adj_off is
 * one array over all graphs' nodes, from 0).  The answer is the removed edges in removal order, each as the edge list of the
 * graph names it (u < v, local indices): removed_u / removed_v [removed_off[j] .. removed_off[j + 1]).  A graph without an edge
 * gets no removal.  The sequence equals, exactly and in order, what the Python loop removes: all arithmetic in doubles, no fused
 * multiply-add, every sum in the order Brandes' algorithm as networkx wrote it adds.
 * PDL_ERR_ARGUMENT, before any index is used: NULL pointers, n_graphs == 0, offsets that do not start at 0 or decrease, a
 * neighbour index outside its graph, a self loop, a neighbour named twice, an edge present in one direction only.
 * PDL_ERR_UNSUPPORTED: 2^31 nodes or adjacency slots and more; a graph whose scratch does not fit option "split_scratch_bytes"
 * (default 2^30; a batch is cut into chunks of graphs under it).  Needs no preprocess and changes nothing of the context: scores,
 * edges, families and pdl_timings stay as they were.  Free with pdl_free_split. */
typedef struct {
    uint32_t graphs, chunks;  /* graphs of the call; launches it was cut into */
    uint64_t nodes, edges;    /* over all graphs (an edge counts once) */
    uint64_t removals;        /* removed_off[graphs] */
    uint64_t rounds;          /* betweenness computations over all graphs (= removals: every round removes one edge) */
    uint64_t *removed_off;    /* [graphs + 1] */
    uint32_t *removed_u;      /* [removals] */
    uint32_t *removed_v;      /* [removals] */
    float device_ms;          /* the launches, between HIP event pairs; validation, uploads and the copies back are not in it */
} pdl_split;
PDL_API int pdl_split_first_level(pdl_ctx *, uint32_t n_graphs, const uint64_t *node_off /* [n_graphs + 1] */,
                                  const uint64_t *adj_off /* [nodes + 1] */, const uint32_t *adj, pdl_split *out);
PDL_API void pdl_free_split(pdl_split *);

/* ---- Pan-genome profile: the family table of a labelling, and pan / core accumulation curves over genome orders -------------
 * What example/quality.py counts over a .clus, and the curve every pan-genome study draws behind it.  pdl_family_profile takes a
 * caller's labelling: a family is the set of genes with equal family_of; any label in [0, n_sequences) is accepted, it need not
 * be the smallest member, a gene in no family carries a label of its own.  The F families come in ascending label order; per
 * family its label, size (genes) and spread (distinct genomes), and as a CSR the genomes it has a gene in (ascending inside a
 * family) with the copies it has there: genomes / copies [genome_off[f] .. genome_off[f + 1]).  Over the set: size_hist[s] =
 * families of s genes (s <= max_size), spread_hist[s] = families in s genomes (s <= G), spread_by_genome[s * G + g] = families
 * of spread s that genome g takes part in; core (spread = G), single_copy_core (spread = G = size), unique (spread = 1),
 * accessory (neither; with one genome a family is core and unique at once).  Per genome: its genes, and those of them in core,
 * accessory and unique families.
 * PDL_ERR_ARGUMENT: NULL pointers, n_sequences == 0, n_genomes == 0, a label >= n_sequences or a genome id >= n_genomes (counted
 * on the device and read by the host before any id indexes anything; the message names the count).  PDL_ERR_UNSUPPORTED: 2^31
 * genes and more, more than 8192 genomes (spread_by_genome has (G + 1) * G entries).  Any state of the context is accepted and
 * nothing of it changes: scores, edges, families and pdl_timings stay as they were.  Free with pdl_free_profile. */
typedef struct {
    uint32_t n_sequences, n_genomes;  /* N, G of the call */
    uint32_t families;                /* F */
    uint32_t incidences;              /* genome_off[F]: (family, genome) pairs with a gene */
    uint32_t max_size;
    uint32_t core, single_copy_core, unique, accessory;
    uint32_t *label, *size, *spread;  /* [F] */
    uint32_t *genome_off;             /* [F + 1] */
    uint32_t *genomes, *copies;       /* [incidences] */
    uint32_t *size_hist;              /* [max_size + 1] */
    uint32_t *spread_hist;            /* [G + 1] */
    uint32_t *spread_by_genome;       /* [(G + 1) * G] */
    uint32_t *genome_genes, *genome_core, *genome_accessory, *genome_unique;     /* [G] genes of the genome; ... in families of that class */
    float device_ms;                  /* the launches, between HIP event pairs; uploads and the copies back are not in it */
} pdl_profile;
PDL_API int pdl_family_profile(pdl_ctx *, const uint32_t *family_of /* [n_sequences] */, const uint32_t *genome_of /* [n_sequences] */,
                               uint32_t n_sequences, uint32_t n_genomes, pdl_profile *out);
PDL_API void pdl_free_profile(pdl_profile *);

/* pdl_pan_curves: for every one of n_orders genome orders (orders[o * G .. o * G + G), each a permutation of 0..G-1; G =
 * profile->n_genomes) pan[o * G + i] = families with a gene in at least one of the genomes orders[o][0..i], core[o * G + i] =
 * families with a gene in every one of them.  Exact integers: pan[o][G-1] = F, core[o][G-1] = profile->core, pan[o][0] =
 * core[o][0].  Of the profile the call reads n_genomes, families, incidences, core, spread, genome_off and genomes.  The device
 * takes no random numbers: the orders are the caller's.
 * PDL_ERR_ARGUMENT: NULL pointers, n_orders == 0; a profile whose fields contradict each other (no family or genome, offsets
 * that do not run from 0 to incidences, a row that is not spread[f] ascending genome ids below G, a core count that is not the
 * number of rows of G genomes); an order that is no permutation (an id >= G or an id named twice: counted on the device before
 * an order indexes anything, the message names the first failing order).  PDL_ERR_UNSUPPORTED: G above PDL_PAN_MAX_GENOMES (the
 * order, its inverse and two histograms of G + 1 bins sit in one workgroup's LDS), 2^31 values per curve and more.  Any state of
 * the context, nothing of it changes.  Free with pdl_free_curves. */
#define PDL_PAN_MAX_GENOMES 4096
typedef struct {
    uint32_t n_genomes, n_orders, families;
    uint32_t incidences;
    uint32_t *pan, *core;             /* [n_orders * n_genomes] */
    float device_ms;
} pdl_curves;
PDL_API int pdl_pan_curves(pdl_ctx *, const pdl_profile *profile, const uint32_t *orders /* [n_orders * G] */, uint32_t n_orders,
                           pdl_curves *out);
PDL_API void pdl_free_curves(pdl_curves *);

/* ---- Genome-by-genome shared-family matrices of a profile ------------------------------------------------------------------
 * How much gene content any two genomes share — what gene-content trees and heat maps are drawn from.  With G =
 * profile->n_genomes, both matrices row-major with both triangles filled:
 *   shared[g * G + h]         families with a gene in g and in h; the diagonal: the families genome g takes part in
 *   shared_copies[g * G + h]  sum over the families of min(copies in g, copies in h), the multiset Jaccard's numerator over the
 *                             families' copy numbers; the diagonal: the genes of g (the profile's genome_genes[g])
 * A genome without a gene has a zero row and a zero column.  Exact integers: with the copy counts in unary bit columns
 * (min(a, b) = sum over t >= 1 of [a >= t][b >= t]) both are AND-popcount products of one bit matrix of levels = 64 * ceil(F / 64)
 * + sum over the families of (largest copy count - 1) columns per genome, worked through in slabs of at most option
 * "matrix_slab_bytes" (default 2^28; a slab is at least one 64-bit word per genome wide) and, inside a slab, in `splits` parts of
 * its words per pair of 64-genome tiles.  Of the profile the call reads n_sequences, n_genomes, families, incidences, core, size,
 * spread, genome_off, genomes and copies.
 * PDL_ERR_ARGUMENT (out is zeroed): NULL pointers; a profile whose fields contradict each other — what pdl_pan_curves refuses,
 * and a copy count of 0, a row whose copies do not add up to size[f], sizes that do not add up to n_sequences.
 * PDL_ERR_UNSUPPORTED: more than 8192 genomes, 2^31 incidences and more, 2^32 bit columns and more.  Any state of the context,
 * nothing of it changes.  Free with pdl_free_genome_matrix.  (The struct carries the call's name as its tag: C keeps tags apart
 * from functions, so it is written `struct pdl_genome_matrix`.) */
struct pdl_genome_matrix {
    uint32_t n_genomes, families, incidences;
    uint32_t levels;                  /* L: bit columns per genome */
    uint32_t slabs;                   /* slabs that were run */
    uint32_t splits;                  /* the largest number of parts a slab's words were cut into */
    uint32_t *shared, *shared_copies; /* [n_genomes * n_genomes] */
    float device_ms;                  /* the launches, between a HIP event pair; validation, uploads and the copies back are not in it */
};
PDL_API int pdl_genome_matrix(pdl_ctx *, const pdl_profile *profile, struct pdl_genome_matrix *out);
PDL_API void pdl_free_genome_matrix(struct pdl_genome_matrix *);

/* ---- place: a new genome's genes in the gene families already built, without a commit -------------------------------------
 * pdl_place_query: the base context holds N genes in G genomes; the query is n_query genes taken as genome G with ids
 * N..N+n_query-1 in union numbering, exactly as pdl_query_scores does.
 * Edges: src/dst/score are the addConnection calls of task G in the union run — Pangenes.java:98-176 applied to the block
 * pdl_query_scores returns, filtered on the device where the block lies — in the host's insertion order: phase 1 cell by cell,
 * (row, col) then (col, row), then phase 2; edges_phase1 of them are phase 1.  Bit for bit and in order what
 * pangenes.bbh_edges(block) gives on the host and what pdl_compute_edges(G) gives on a context the same genes were appended to.
 * Placement: the combined network is the base network as the context has it (pdl_compute_edges over all genomes) plus the
 * query's edges.  Components, labels, node-ness and collisions follow pdl_families: edges are undirected, a repeated pair is one
 * edge, a self edge makes its gene a node but is no edge, a label is the smallest gene id of the component, a component collides
 * when it holds two genes of one genome that are not adjacent.  Only the part the query touches is returned:
 *   family_of[n]     label of each query gene's combined component: a base gene id when the component holds base genes, a query
 *                    id >= N for a family of query genes only, the gene's own id for a gene without an edge
 *   is_node[n]       the query gene has an edge (self edges count)
 *   groups           the combined components that hold at least one query node, in ascending label order; per group its label,
 *                    its query members ascending (group_query_off / group_query, union ids) and the labels of the base
 *                    components it fuses, ascending (group_base_off / group_base; a base gene that was no node in the base counts
 *                    as a component of one).  No base component: a novel family; one: the genes join it; two or more: a bridge.
 *   group_collides   the collision flag of the whole combined component = a fused base component already collides, OR two
 *                    distinct fused base components hold genes of one genome (they cannot be adjacent: every new edge has a
 *                    query end), OR the group's m >= 2 query genes are not a clique under the phase-2 edges
 *   novel, joined, bridging, colliding: groups of each kind; unplaced: query genes without an edge
 *   device_ms        as pdl_query_info.device_ms, over the query and the placement
 * NOT the families of a union rebuild, in two ways, neither of which is attempted: (1) the base genomes' paralog thresholds
 * (Pangenes.java:146-155) can only fall once genome G exists, so a union run may add intra-genome edges between base genes;
 * (2) the union's last-record fold (library.cpp:297-306) can change single base-to-base cells.  pdl_append_genomes commits.
 * The base context is only read: scores, edges, families, dictionary, costs and timings are equal before and after, placements
 * are independent of each other; the context's families are computed on first use, as by pdl_compute_families.  Refusals are
 * decided before anything is returned and leave `out` zeroed: every state pdl_query_scores refuses and every state
 * pdl_compute_families refuses (a genome shard in force included) is PDL_ERR_STATE; the query's argument and domain refusals pass
 * through with their codes and messages.  `info` (may be NULL): the query's own sizes, as pdl_query_scores fills it.
 * pdl_placement_of_edges: the same kernels over a caller's query edge list in union ids, on a caller's base — `base` as
 * pdl_compute_families / pdl_families_of_edges returned it for the N = base->sequences base genes, genome_of[N] their genomes (the
 * query is one further genome).  The list is read as pdl_families_of_edges reads one: any order, repeats, both directions and
 * self edges allowed, query-query pairs de-duplicated before they are counted.  src/dst/score of `out` stay NULL.  Of the context
 * only the device, the stream and work buffers are used.  PDL_ERR_ARGUMENT, counted on the device BEFORE any id indexes
 * anything: an id outside [0, N + n_query), an edge with both ends below N; also NULL pointers, n_query == 0 and a `base` whose
 * fields contradict each other.  Free with pdl_free_placement. */
typedef struct {
    uint32_t sequences;        /* N of the base */
    uint32_t n_query;          /* n */
    uint32_t genomes;          /* G: the query's genome id */
    uint32_t edges;            /* pdl_place_query: the query's edges ... */
    uint32_t edges_phase1;     /* ... of which phase 1 (the first edges_phase1 entries) */
    uint32_t groups;
    uint32_t novel, joined, bridging, colliding, unplaced;
    float device_ms;
    int32_t *src, *dst;        /* [edges] union ids */
    float *score;              /* [edges] */
    uint32_t *family_of;       /* [n] */
    uint8_t *is_node;          /* [n] */
    uint32_t *group_label;     /* [groups] ascending */
    uint32_t *group_query_off; /* [groups+1] into group_query */
    uint32_t *group_query;     /* query genes (union ids), ascending inside a group */
    uint32_t *group_base_off;  /* [groups+1] into group_base */
    uint32_t *group_base;      /* labels of the fused base components, ascending inside a group */
    uint8_t *group_collides;   /* [groups] */
} pdl_placement;
PDL_API int pdl_place_query(pdl_ctx *, const uint8_t *residues, const uint64_t *offsets /* [n_query+1] */, uint32_t n_query,
                            pdl_placement *out, pdl_query_info *info /* may be NULL */);
PDL_API int pdl_placement_of_edges(pdl_ctx *, const pdl_families *base, const uint32_t *genome_of /* [base->sequences] */, uint32_t n_query,
                                   const int32_t *src, const int32_t *dst, uint64_t n_edges, pdl_placement *out);
PDL_API void pdl_free_placement(pdl_placement *);

/* ---- place, for a batch: q new genomes placed in one pass, each on its own --------------------------------------------------
 * pdl_place_batch: the n genes are cut into queries exactly as pdl_query_batch cuts them (gene_begin [n_queries + 1], from 0 to
 * n, strictly increasing).  out[j] equals, field for field and byte for byte, what pdl_place_query returns for the genes of query
 * j alone on the same context; only device_ms differs (an even share of its chunk's).  All ids in out[j] are query j's own union
 * ids: its genes are N..N+n_j-1 of genome G, a novel family's label is its smallest query id in that numbering.  The queries
 * never see each other: two that touch the same base component each get that component and do not fuse.  The base context is
 * only read; its families are computed on first use, as by pdl_compute_families.  info[j] is filled as pdl_query_batch fills it.
 * The queries are scored a chunk at a time (option "query_batch_bytes", as pdl_query_batch) and the best-hit filter runs once
 * over a chunk's cells where they lie; only edges and the placements' small arrays come to the host.
 *
 * Refusals are decided before anything is returned; they leave every out[j] zeroed and the context as it was: every state
 * pdl_place_query refuses (PDL_ERR_STATE), every argument and domain refusal of pdl_query_batch with its code (the absent-byte
 * message names the first such query; option "query_rekey" accepts such bytes as for pdl_query_batch).  A refusal found in a later
 * chunk returns nothing of the earlier chunks.  Each out[j] is
 * freed with pdl_free_placement.
 *
 * pdl_placement_batch_of_edges: the batch form of pdl_placement_of_edges — one caller's base and n_queries edge lists laid end
 * to end, list j = [edge_begin[j], edge_begin[j+1]) in query j's own union ids [0, N + n_query[j]).  out[j] equals
 * pdl_placement_of_edges on list j alone (src / dst / score NULL).  The ids of every list are checked on the device, in one
 * launch, before any id indexes anything: a list that names an id outside its own [0, N + n_query[j]) — which may be valid for a
 * larger query of the same batch — or holds an edge with both ends below N gives PDL_ERR_ARGUMENT, and the message names the first
 * failing query.  NULL pointers, n_queries == 0, an n_query[j] == 0, a decreasing edge_begin or a base whose fields contradict
 * each other: PDL_ERR_ARGUMENT. */
typedef struct {
    uint32_t queries, chunks;
    float device_ms;           /* the chunks' device time: queries, best-hit filter and placements */
} pdl_place_batch_info;
PDL_API int pdl_place_batch(pdl_ctx *, const uint8_t *residues, const uint64_t *offsets /* [n+1] */,
                            const uint32_t *gene_begin /* [n_queries+1] */, uint32_t n, uint32_t n_queries,
                            pdl_placement *out /* [n_queries], each freed with pdl_free_placement */,
                            pdl_query_info *info /* [n_queries] or NULL */, pdl_place_batch_info *binfo /* may be NULL */);
PDL_API int pdl_placement_batch_of_edges(pdl_ctx *, const pdl_families *base, const uint32_t *genome_of /* [base->sequences] */,
                                         uint32_t n_queries, const uint32_t *n_query /* [n_queries] genes of each query */,
                                         const uint64_t *edge_begin /* [n_queries+1] */, const int32_t *src, const int32_t *dst,
                                         pdl_placement *out /* [n_queries] */);

/* Number of emitted cells per genome after pdl_score_all ([G], 0 for genomes outside the shard) */
PDL_API int pdl_scores_counts(pdl_ctx *, uint32_t *out_counts);

/* Parity-test introspection: the dictionary in (rank, gene) order as library.cpp:270-287 leaves it
 * (before the group scan's re-sort of the folded last group).  Arrays sized by pdl_cost.dictionary_records. */
PDL_API int pdl_get_dictionary(pdl_ctx *, uint64_t *ranks, uint32_t *seqs, uint32_t *counts);
/* Alphabet rank table (library.cpp:96-99) and B^(k-1) (library.cpp:101-119) */
PDL_API int pdl_get_rank_table(const pdl_ctx *, uint8_t out_rank_values[256], uint64_t *out_last_multiplier);

PDL_API int pdl_get_timings(pdl_ctx *, pdl_timings *out);

/* Tuning / test switches of one context (no environment variable is read by the library).  Unknown names fail with
 * PDL_ERR_ARGUMENT.  Options: "join_tier1" 0|9|10|11|20|21 (table of the join's first tier; -1 = default: by genome count),
 * "join_tier0" -1|0|1 (the partition tier in front of tier 1 — several short rows per workgroup cycle, no hash table: -1 = by the
 * average row length, the default; it stays off when "join_tier1" was set by hand unless forced with 1),
 * "sift_threshold" 0|1 (that tier's sift: 1, the default = a column goes to the table only when the cycle's counter of it reached
 * what the set's shortest gene would need to emit it — on sets where that threshold is 4 or more; below it, i.e. with a gene of
 * at most 6k k-mers in the set, the sift is "seen twice" on two bitmaps, as it was before the counters; 0 = the counters with the
 * threshold forced to 2: a test switch, several times slower on large sets; the scores are the same either way; any other value
 * is rejected),
 * "join_tiny_tier2" 0|1 (512-slot second tier, so that small test sets reach the HBM-table kernel), "host_mirror" 0|1
 * (pdl_compute_scores slices ONE pinned copy of the whole result (1, default) or copies each genome's block from the
 * device (0); results above 1 GiB always take the second way), "staging_cap" n (cells of staging the first scoring
 * attempt may use, 0 = estimate; a pass that overflows it is repeated once with the exact size), "join_grid_pct" n (first
 * tier of the join launched with n % of the workgroups the chip holds, 0 = all: an experiment knob — how the join scales
 * with rows in flight), "stage_timers" 0|1 (default 1: HIP events around every stage fill the stage
 * fields of pdl_timings; 0: only the totals and the join's launch time are taken — each event pair is two marker packets
 * between dispatches, a few microseconds of idle stream on a two-millisecond step), "low_memory" 0|1 (for genome batches on a large set: the buffers only the dictionary build needed are released after it —
 * pdl_get_dictionary is then not available — and tier 3's tables in HBM take 1 GB instead of 8), "query_batch_bytes" n > 0
 * (device bytes one chunk of pdl_query_batch / pdl_place_batch may take before its join, default 2^30), "split_scratch_bytes" n > 0 (device bytes of scratch one launch of
 * pdl_split_first_level may take, default 2^30; it too leaves the context's scores in place), "matrix_slab_bytes" n > 0 (device bytes the genomes' bit rows of
 * one slab of pdl_genome_matrix may take, default 2^28; at least one word per genome; it too leaves the scores in place), "onepass_scan" 0|1 (prefix scans
 * in one launch with decoupled look-back instead of three launches; measured slower on MI355X, default 0), "lean_radix" 0|1
 * (default 1: the offsets of a radix pass come from one launch, a workgroup per digit, and the kernel that ranks the k-mers files
 * the rank sort's first histogram — whole-stream single-GPU builds with exact ranks, tables of at most 65 536 tiles, "onepass_scan"
 * off; 0: a histogram kernel and a three-launch scan for every pass.  Same results either way: for parity tests and A/B timing),
 * "lean_records" 0|1 (default 1: the passes of a build that run once over the sorted k-mers and over the records load each of them
 * once and take a neighbour's value from the neighbouring lane — the run-length pass in kernels of its own, the range count on bit
 * masks — and the one-workgroup launch in the middle of a three-launch scan stages its sums through LDS; 0: the former kernels.
 * Same results either way: for parity tests and A/B timing),
 * "order_offsets" 0|1|2 (default 2: the cell offsets of a scoring pass with upper-triangle range lists come from one launch of
 * several workgroups; 1: of one workgroup; 0: from two prefix scans, four launches.  Same results: for parity tests and A/B timing),
 * "order_offsets_rows" n (that launch serves at most n task rows, default and maximum 131 072; tests lower it),
 * "order_subwave" 0|1|16|32 (default 1 = 16: a wave of the kernel that puts the cells in emission order takes 64 / W rows, each in a
 * segment of W lanes, and the mirrored cells are handed on W lanes per source row; 0: a wave per row), "order_wide_merged" 0|1
 * (default 1: the rows of more than 256 cells are sorted by workgroups of that same launch; 0: by a launch of their own),
 * "fused_glue" 0|1|n (default 1: the descriptors and the clearing that open the first scoring pass are one launch, and so are the
 * genes' range offsets and the per-genome costs that close a build; 0: one launch each; n > 1: as 1, and the k-mer counts of the
 * genes with the clearing of the control block in one launch for up to min(n, 65 536) genes, measured slower.  Same results for all three: for parity
 * tests and A/B timing),
 * "aside_test_reload" 0|1 (test switch: the next scoring pass
 * behaves as if an entry of a put-aside list had needed a second look, so the repeat with fully tagged entries runs),
 * "alphabet_rekey" 0|1 (default 0: pdl_append_genomes / pdl_remove_genomes go through where the alphabet changes, by writing the
 * sorted stream's keys again; set BEFORE pdl_preprocess it also makes the build record the letters of genes shorter than k, one
 * small launch more, which an exact removal needs — see pdl_get_rekey_info; like "query_batch_bytes" it leaves the context's
 * scores in place), "query_rekey" 0|1 (default 0: pdl_query_scores, pdl_query_batch, pdl_place_query and pdl_place_batch accept
 * query bytes the base's alphabet lacks by ranking the query in the union's alphabet — see pdl_get_query_rekey_info; it too leaves
 * the context's scores in place and, like every option, outlives a rebuild). */
PDL_API int pdl_set_option(pdl_ctx *, const char *name, int64_t value);

/* ---- multi-GPU: one context per GPU, the caller moves bytes between them (RCCL over xGMI) -----------------------
 * Counterpart of the reference's per-genome tasks on a thread pool over ONE shared dictionary (Pangenes.java:54-66,
 * library.cpp:73): here every GPU holds the whole dictionary, built co-operatively, and scores a disjoint set of genomes.
 * All ranks call the same sequence with the SAME input (every host reads the .faa); nothing below communicates by
 * itself — the caller owns the collectives (pandelos_amd/distributed.py: torch.distributed):
 *
 *   pdl_dist_preprocess_begin   histogram, rank table, k-mer ranks (every rank, from the shared input); the rank space is
 *                               cut into `world` intervals of ~equal k-mer counts (same cuts on every rank: they depend on
 *                               the input only) and this rank sorts + dedups ITS interval (library.cpp:270-287 on 1/world
 *                               of the records).  Result: its run of the dictionary, pdl_dist_slice.
 *   -- caller: all-gather the record counts, then the runs themselves into ONE device array in rank order
 *      (the concatenation IS the dictionary in (rank, gene) order: no merge) --
 *   pdl_dist_preprocess_finish  adopts that array (must stay valid until the next preprocess), deals the genomes to ranks
 *                               (longest-processing-time on each genome's lookups above the diagonal: identical input,
 *                               identical deal on every rank) and builds the rank-groups and posting-range lists
 *                               (library.cpp:289-335) of this rank's genes.
 *   pdl_dist_score_begin        scores this rank's rows against the genes ABOVE them only; a cell whose column belongs to
 *                               another rank's genome is also that rank's cell (c, r) (same sums, perc/tr_perc swapped):
 *                               such cells are listed per destination rank, pdl_dist_outbox.
 *   -- caller: all-to-all the per-destination counts, then the 24-byte cells --
 *   pdl_dist_score_finish       files the received cells with the local ones, folds them into the per-(row, genome) and
 *                               per-column maxima and puts every row in the reference's emission order.
 * Afterwards pdl_compute_scores / pdl_scores_counts work for the genomes of this rank (pdl_dist_genome_owner).
 * pdl_genome_cost and pdl_cost.total_cost cover this rank's genomes only (the reference prints "Genome g cost" from the
 * task that scores g, library.cpp:535-538); "Total cost" is their sum over the ranks — a scalar all-reduce of the caller.
 * The counters over the dictionary (records, shared records, groups) are complete on every rank. */
typedef struct {
    const void *d_postings;   /* device, records x 8 bytes {gene u32, count u32 | group-head flag in bit 31} */
    uint64_t records;         /* unique (rank, gene) records of this rank's interval */
    uint64_t kmers;           /* k-mer occurrences of this rank's interval */
    const uint64_t *genome_weights; /* host, [genomes]: every genome's lookups above the diagonal inside this run; summed over
                                 the ranks they are the weights of the genome deal; valid until the next call on this context */
    uint32_t genomes;
    const uint64_t *genome_costs;   /* host, [genomes]: every genome's lookups inside this run as the reference counts them (library.cpp:327);
                                 summed over the ranks: "Genome g cost" (exact whenever pdl_dist_preprocess_ranges says "available") */
} pdl_dist_slice;

/* Range lists built by the senders (the default flow of pandelos_amd/distributed.py).  pdl_dist_preprocess_finish makes every rank
 * walk the whole gathered dictionary twice to find the ranges of its own genes — work that does not shrink with the number of
 * ranks.  Groups never straddle runs, so between begin and finish each rank can make the range tuples of ALL genes of its run
 * (library.cpp:289-335 on 1/world of the records) and file them by the rank that owns the gene:
 *
 *   pdl_dist_preprocess_begin
 *   -- caller: all-gather [records | genome_weights | genome_costs] --
 *   pdl_dist_preprocess_ranges         deals the genomes (as _finish would), builds + files the tuples of this run
 *   -- caller: all-gather [counts[world] | shared_records | groups | repeat_sample]; all-to-all the tuples (keys: 4 bytes, ranges:
 *      8 bytes, same split sizes); the runs into one device array as before (this call only reads the run: the group-head bits
 *      travel with it, every reader of a count masks bit 31; libraries before that took them out here, so the flow gathers AFTER) --
 *   pdl_dist_preprocess_finish_ranges  adopts the dictionary, sorts the received tuples (source-rank major) by gene
 *
 * `available` = 0 (gene ids beyond 22 bits, more than 256 ranks, a last run of exactly one record — the same verdict on every rank:
 * it depends on the input and the record counts only): nothing was built, the caller goes on with pdl_dist_preprocess_finish.
 *
 * Refusals (none of them damages the build or the pass: the contexts go on from where they stood, or from the call named here).
 * PDL_ERR_STATE: any of these calls out of the order above — also pdl_dist_preprocess_ranges a second time on a run whose tuples it
 * has built, and pdl_dist_preprocess_finish after it.  PDL_ERR_ARGUMENT: world 0 or above 64, rank >= world, NULL or misaligned
 * arrays, record counts that do not add up to the runs; and what a peer could not have sent, counted on the device before it is
 * used — a tuple whose key is not (this rank << 24 | a gene of this rank's genomes) or whose range ends past the gathered
 * dictionary, tuples for a rank that owns no gene (then: pdl_dist_preprocess_begin again); a cell whose row or column is no gene
 * or whose column is not a row of this rank (then: pdl_dist_score_begin again), cells for a rank without rows. */
typedef struct {
    int available;
    const uint32_t *d_keys;         /* device, tuples grouped by destination rank, record order inside: (owner << 24 | gene) */
    const uint64_t *d_ranges;       /* device, {first posting in the GATHERED dictionary, postings | min(own count, 1023) << 22} */
    const uint64_t *counts;         /* host, [world]: tuples for each rank; valid until the next call on this context */
    uint64_t total;
    uint64_t shared_records, groups, repeat_sample;   /* counters over this run; the caller hands their sums over the ranks to _finish_ranges */
} pdl_dist_ranges;

typedef struct { float score, perc, tr_perc; uint32_t row, column, first_group; } pdl_dist_cell;   /* cell (row, column) as its row's rank computed it */

typedef struct {
    const pdl_dist_cell *d_cells;  /* device, grouped by destination rank in rank order */
    const uint64_t *counts;        /* host, [world]: cells for each rank (0 for this rank itself); valid until the next call on this context */
    uint64_t total;
} pdl_dist_outbox;

PDL_API int pdl_dist_preprocess_begin(pdl_ctx *, const uint8_t *d_residues, const uint64_t *d_offsets, const uint32_t *d_genome_of,
                                      uint32_t n_sequences, uint64_t n_residues, int kvalue, uint32_t world, uint32_t rank,
                                      pdl_dist_slice *out);
/* genome_weights: [G], the element-wise sum of every rank's pdl_dist_slice.genome_weights (one small all-reduce beside
 * the record counts) — the SAME vector on every rank; NULL: the library takes one more pass over the gathered
 * dictionary and computes them itself. */
PDL_API int pdl_dist_preprocess_finish(pdl_ctx *, void *d_postings_all, uint64_t total_records, const uint64_t *genome_weights /* may be NULL */,
                                       pdl_cost *out_cost /* may be NULL */);
/* run_records: [world] records of every rank's run; genome_weights / genome_costs: [G] element-wise sums over the ranks */
PDL_API int pdl_dist_preprocess_ranges(pdl_ctx *, const uint64_t *run_records, const uint64_t *genome_weights, const uint64_t *genome_costs,
                                       pdl_dist_ranges *out);
/* d_keys / d_ranges: the received tuples, source-rank major (what all_to_all leaves); they are sorted in place / into library
 * memory and must stay valid, like d_postings_all, until the next preprocess.  counter_sums: [3] shared_records, groups,
 * repeat_sample summed over the ranks.  pdl_genome_cost then answers for every genome; pdl_sequence_costs is not available. */
PDL_API int pdl_dist_preprocess_finish_ranges(pdl_ctx *, void *d_postings_all, uint64_t total_records, uint32_t *d_keys, uint64_t *d_ranges,
                                              uint64_t n_tuples, const uint64_t *counter_sums /* [3] */, pdl_cost *out_cost /* may be NULL */);
PDL_API int pdl_dist_genome_owner(const pdl_ctx *, uint32_t *out_owner /* [G] */);
PDL_API int pdl_dist_score_begin(pdl_ctx *, pdl_dist_outbox *out);
PDL_API int pdl_dist_score_finish(pdl_ctx *, const pdl_dist_cell *d_inbox, uint64_t n_inbox);
/* dst[0..bytes) = src[0..bytes), both on this context's device, queued on its stream and waited for (the runs and
 * outboxes above live in library-owned memory, the exchange buffers in the caller's). */
PDL_API int pdl_copy_device(pdl_ctx *, void *d_dst, const void *d_src, uint64_t bytes);

/* Test hooks of the small device->host read protocol (a kernel stores counters straight into pinned host memory, then a
 * checksum and an epoch flag; the host spins on both: pandelos_amd/csrc/pdl_common.h, PinRead), on plain host memory:
 * pdl_pin_checksum = what the kernel leaves beside the flag for a payload; pdl_pin_arrived = 1 when `pin` shows `epoch` at
 * flag_word and the words of the n segments (dst_word[s] .. + words[s]) add up to the checksum at flag_word + 1. */
PDL_API int pdl_pin_arrived(const uint32_t *pin, const uint32_t *dst_word, const uint32_t *words, uint32_t n, uint32_t flag_word, uint32_t epoch);
PDL_API uint32_t pdl_pin_checksum(const uint32_t *payload, const uint32_t *dst_word, const uint32_t *words, uint32_t n);

/* Test hooks of the generic device primitives (pandelos_amd/csrc/pdl_hooks.hip): each runs one primitive as the library calls
 * it, on the caller's device buffers, on the context's stream, and waits for it.  The form taken follows the options
 * onepass_scan, lean_radix and lean_records.  For a context that holds no build: PDL_ERR_STATE on one that does (the scratch buffers the hooks
 * grow are the build's); PDL_ERR_ARGUMENT for a NULL where a pointer is needed or a width that is not listed.
 *
 * pdl_test_scan: scan_and_apply over d_flags[0 .. min(*d_n, n_bound)) — d_prefix[i] = exclusive prefix, d_seen_flag[i] = the flag
 * the apply step was handed; two_phase: an apply functor of the load/store form, which reads d_flags[i] again and sets bit 31 of
 * d_seen_flag[i] where that differs.  *d_total (and *d_total2, which may be only 4-byte aligned) = the sum.  With onepass_scan
 * the look-back error word is read and a set one fails the call with PDL_ERR_DEVICE.
 * pdl_test_radix_offsets: pdl_radix_offsets over d_counts[256][n_tiles].  *out_lean = 1: d_offs holds each row's own exclusive
 * prefix and d_digit_total[256] the rows' sums (*d_total is not written); 0: d_offs is the exclusive prefix over the whole
 * table, *d_total its sum (d_digit_total is not written).
 * pdl_test_sort_pairs: pdl_sort_pairs for (key_bytes, val_bytes) = (4, 4), (8, 4), (4, 8); begin_bit a multiple of 8.
 * d_first_counts [256][tiles of 4096], on the device: filed at the head of the sort's scratch as the first pass's histogram.
 * *out_result_in_b = 1 when the sorted pairs are in (d_keys_b, d_vals_b); *out_total = the control block's total of the last
 * pass (all ones where no pass ran).
 * pdl_test_merge: pdl_merge_streams for key_bytes 4 | 8: the stable merge of a and b on key & mask, a first on ties, b's
 * values + b_val_add.  Sources need element alignment only, the outputs 16 bytes. */
PDL_API int pdl_test_scan(pdl_ctx *, const uint32_t *d_flags, uint64_t n_bound, const uint64_t *d_n /* may be NULL */, uint32_t *d_prefix,
                          uint32_t *d_seen_flag, int two_phase, uint64_t *d_total, uint64_t *d_total2 /* may be NULL */);
PDL_API int pdl_test_radix_offsets(pdl_ctx *, const uint32_t *d_counts, uint32_t *d_offs, uint32_t n_tiles, uint64_t *d_total,
                                   uint32_t *d_digit_total /* [256] */, int *out_lean);
PDL_API int pdl_test_sort_pairs(pdl_ctx *, uint32_t key_bytes, uint32_t val_bytes, void *d_keys_a, void *d_keys_b, void *d_vals_a, void *d_vals_b,
                                uint64_t n, uint32_t end_bit, int iota_values, const uint64_t *d_n /* may be NULL */, uint32_t begin_bit,
                                int keys_below_end_bit, const uint32_t *d_first_counts /* may be NULL */, int *out_result_in_b, uint64_t *out_total);
PDL_API int pdl_test_merge(pdl_ctx *, uint32_t key_bytes, const void *d_a_keys, const uint32_t *d_a_vals, uint32_t na, const void *d_b_keys,
                           const uint32_t *d_b_vals, uint32_t nb, uint32_t b_val_add, uint64_t mask, void *d_out_keys, uint32_t *d_out_vals);

/* Library/build identification, e.g. "pandelos_amd 0.2 (HIP, gfx950)" */
PDL_API const char *pdl_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PANDELOS_AMD_H */
