// pdl_state.h — what a context's state words mean: the one reset ("these results are stale") and the one gate ("this entry
// point needs that state") every entry point of pdl_api.hip and pdl_ingest.hip goes through.  Included by pdl_common.h behind
// pdl_ctx; plain members are all it reads and writes (tools/state_gate_check.cpp runs it without a device).
#pragma once

// ---- the reset -----------------------------------------------------------------------------------------------------------------
// How much of a context goes stale, deepest first; each depth drops what the next one drops, and more:
//
//   depth             preprocessed  tasks_ready  reshard_pending  scored  mirror / edges / fam  plans (qb, qbb, pb)  U Ushared NG P M  multi-GPU words
//   set               false         false        false            false   false                 renewed              0                cleared
//   build             false         false        false            false   false                 -                    -                -
//   scores_and_tasks  -             false        -                false   false                 -                    -                -
//   scores            -             -            -                false   false                 -                    -                -
//
// `set`: another set is coming (every build entry point, pdl_dist_preprocess_begin).  The multi-GPU words are dist, dist_stage,
// dist_sender, post_ext — and the deal of a multi-GPU build (shard, shard_set), which does not carry over; a caller's genome shard
// and the options stay in force.  `build`: the dictionary is about to change under the context (an append, a removal, an ingest
// into the buffers a build reads); sizes, plans and key kinds are the caller's to carry over.  `scores_and_tasks`: another genome
// shard.  `scores`: an option changed, or a scoring pass starts.  preprocessed is set again only behind a build that went through,
// scored behind a pass, the three derived products behind their own runs.
enum class Stale { set, build, scores_and_tasks, scores };
inline void pdl_stale(pdl_ctx *c, Stale depth) {
    c->scored = false;
    c->mirror_valid = false; c->edges_valid = false; c->fam_valid = false;
    if (depth == Stale::scores) return;
    c->tasks_ready = false;
    if (depth == Stale::scores_and_tasks) return;
    c->preprocessed = false; c->reshard_pending = false;
    if (depth == Stale::build) return;
    pdl_renew(c->qb); pdl_renew(c->qbb); pdl_renew(c->pb);
    c->U = c->Ushared = c->NG = c->P = c->M = 0;
    if (c->dist) { c->shard.clear(); c->shard_set = false; }
    c->dist = false; c->dist_stage = DistStage::none; c->dist_sender = false; c->post_ext = nullptr;
}

// ---- the gate ------------------------------------------------------------------------------------------------------------------
// What an entry point can need of the context's state.  A need's refusal is PDL_ERR_STATE with the text below (%s: the entry
// point), unless the entry point's row brings its own.
enum Need : unsigned {
    NEED_END = 0,
    NEED_INGESTED,        // pdl_ingest_faa has run                                                       (the row's text)
    NEED_BUILT,           // a build went through                                    "%s before pdl_preprocess"
    NEED_RANGES,          // ... and not with only_complexity: the posting ranges exist  "%s: the context was preprocessed with only_complexity"
    NEED_SINGLE_GPU,      // not a multi-GPU context                                 "%s: not available on a multi-GPU context[ (gather the edges: <edge form>)]"
    NEED_NO_SHARD,        // no genome shard in force: every genome's ranges and edges are here  "%s: not available with a genome shard in force", or the edge form's
    NEED_STREAM,          // the sorted k-mer stream is still held (low_memory releases it)  "%s: the sorted k-mer stream was released (option low_memory)"
    NEED_GENE_COSTS,      // per-gene costs are kept: not a multi-GPU build with sender-built tuples  (the row's text)
    NEED_NO_DEAL,         // no multi-GPU build has begun                                                 (the row's text)
    NEED_AT_SLICE,        // multi-GPU build at stage slice_built                                         (the row's text)
    NEED_ADOPTED,         // multi-GPU build at stage adopted or later                                    (the row's text)
    NEED_AT_JOINED,       // multi-GPU build at stage joined                                              (the row's text)
    NEED_TUPLES,          // pdl_dist_preprocess_ranges built this run's range tuples                     (the row's text)
    NEED_NO_TUPLES,       // ... it did not                                                               (the row's text)
};
enum Entry {
    E_PREPROCESS_INGESTED, E_GENOME_COST, E_SEQUENCE_COSTS, E_GET_RANK_TABLE, E_GET_DICTIONARY, E_SET_GENOME_SHARD, E_SCORE,
    E_DIST_FINISH, E_DIST_RANGES, E_DIST_FINISH_RANGES, E_DIST_GENOME_OWNER, E_DIST_SCORE_BEGIN, E_DIST_SCORE_FINISH,
    E_QUERY_SCORES, E_QUERY_BATCH, E_PLACE_QUERY, E_PLACE_BATCH, E_APPEND_GENOMES, E_REMOVE_GENOMES, E_COMPUTE_FAMILIES,
    E_COUNT
};
struct GateNeed { Need need; const char *text; };        // text: nullptr = the need's own
struct GateRow { Entry entry; const char *who; const char *edge_form; GateNeed needs[6]; };

// Which entry point needs what, in the order it reports what is missing (`=`: at that stage, `>=`: or later):
//
//   entry point                        ingested  built  ranges  single-GPU  no shard  stream  gene costs  multi-GPU stage  tuples
//   pdl_preprocess, _device              -         -      -        -           -        -         -          -              -     (any state: a new set)
//   pdl_dist_preprocess_begin            -         -      -        -           -        -         -          -              -     (any state: a new set)
//   pdl_ingest_faa, pdl_set_option       -         -      -        -           -        -         -          -              -
//   pdl_families_of_edges,               -         -      -        -           -        -         -          -              -     (any state: a caller's edges, graphs,
//     pdl_split_first_level,                                                                                                       labels or orders; the context's own state
//     pdl_family_profile, pdl_pan_curves,                                                                                          is not touched)
//     pdl_genome_matrix
//   pdl_preprocess_ingested             yes        -      -        -           -        -         -          -              -
//   pdl_genome_cost                      -        yes     -        -           -        -         -          -              -
//   pdl_sequence_costs                   -        yes     -        -           -        -        yes         -              -
//   pdl_get_rank_table                   -        yes     -        -           -        -         -          -              -
//   pdl_get_dictionary                   -        yes     -       yes          -       yes        -          -              -
//   pdl_set_genome_shard                 -         -      -        -           -        -         -         = none          -
//   pdl_score_all, pdl_scores_counts,    -        yes    yes      yes          -        -         -          -              -     (asked only of a context that is
//     pdl_compute_scores, _edges                                                                                                   not scored: a scored one serves)
//   pdl_dist_preprocess_finish           -         -      -        -           -        -         -         = slice_built   not built
//   pdl_dist_preprocess_ranges           -         -      -        -           -        -         -         = slice_built   not built
//   pdl_dist_preprocess_finish_ranges    -         -      -        -           -        -         -         = slice_built   built
//   pdl_dist_genome_owner                -         -      -        -           -        -         -         >= adopted      -
//   pdl_dist_score_begin                 -         -      -        -           -        -         -         >= adopted      -
//   pdl_dist_score_finish                -         -      -        -           -        -         -         = joined        -
//   pdl_query_scores, pdl_query_batch    -        yes    yes      yes          -       yes        -          -              -
//   pdl_place_query, pdl_place_batch     -        yes    yes      yes         yes      yes        -          -              -
//   pdl_append_genomes, _remove_genomes  -        yes    yes      yes         yes      yes        -          -              -
//   pdl_compute_families                 -        yes    yes      yes         yes       -         -          -              -
//
// (a query under a genome shard is scored against the whole dictionary; the families need the edges, not the stream; the readers
// of the scores on a multi-GPU context are served once pdl_dist_score_finish has scored it)
#define PDL_NEEDS_QUERY {NEED_BUILT, nullptr}, {NEED_RANGES, nullptr}, {NEED_SINGLE_GPU, nullptr}
static const GateRow PDL_GATE[] = {
    {E_PREPROCESS_INGESTED, "pdl_preprocess_ingested", nullptr, {{NEED_INGESTED, "pdl_preprocess_ingested before pdl_ingest_faa"}}},
    {E_GENOME_COST, "pdl_genome_cost", nullptr, {{NEED_BUILT, nullptr}}},
    {E_SEQUENCE_COSTS, "pdl_sequence_costs", nullptr, {{NEED_BUILT, nullptr},
        {NEED_GENE_COSTS, "per-gene costs are not kept by a multi-GPU build whose range lists came from the senders (pdl_genome_cost works)"}}},
    {E_GET_RANK_TABLE, "pdl_get_rank_table", nullptr, {{NEED_BUILT, nullptr}}},
    {E_GET_DICTIONARY, "pdl_get_dictionary", nullptr, {{NEED_BUILT, nullptr},
        {NEED_SINGLE_GPU, "pdl_get_dictionary: a multi-GPU context keeps ranks only for its own interval"}, {NEED_STREAM, nullptr}}},
    {E_SET_GENOME_SHARD, "pdl_set_genome_shard", nullptr, {{NEED_NO_DEAL, "genome shard: a multi-GPU build deals the genomes itself (pdl_dist_genome_owner)"}}},
    {E_SCORE, "pdl_score_all", nullptr, {{NEED_BUILT, nullptr}, {NEED_RANGES, "the dictionary was built in complexity-only mode (no posting ranges)"},
        {NEED_SINGLE_GPU, "multi-GPU context: score with pdl_dist_score_begin / pdl_dist_score_finish"}}},
    {E_DIST_FINISH, "pdl_dist_preprocess_finish", nullptr, {{NEED_AT_SLICE, "pdl_dist_preprocess_finish without pdl_dist_preprocess_begin"},
        {NEED_NO_TUPLES, "pdl_dist_preprocess_finish after a pdl_dist_preprocess_ranges that built this run's range tuples (and took its group-head bits out): finish with pdl_dist_preprocess_finish_ranges"}}},
    // (a second pdl_dist_preprocess_ranges would count ranges on a run without heads: wrong tuples and counters, and nothing to show for it)
    {E_DIST_RANGES, "pdl_dist_preprocess_ranges", nullptr, {{NEED_AT_SLICE, "pdl_dist_preprocess_ranges without pdl_dist_preprocess_begin"},
        {NEED_NO_TUPLES, "pdl_dist_preprocess_ranges has built this run's range tuples already (and took its group-head bits out): go on with pdl_dist_preprocess_finish_ranges"}}},
    {E_DIST_FINISH_RANGES, "pdl_dist_preprocess_finish_ranges", nullptr,
        {{NEED_AT_SLICE, "pdl_dist_preprocess_finish_ranges without a pdl_dist_preprocess_ranges that said \"available\""},
         {NEED_TUPLES, "pdl_dist_preprocess_finish_ranges without a pdl_dist_preprocess_ranges that said \"available\""}}},
    {E_DIST_GENOME_OWNER, "pdl_dist_genome_owner", nullptr, {{NEED_ADOPTED, "pdl_dist_genome_owner before pdl_dist_preprocess_finish: the genomes have not been dealt"}}},
    {E_DIST_SCORE_BEGIN, "pdl_dist_score_begin", nullptr, {{NEED_ADOPTED, "pdl_dist_score_begin before pdl_dist_preprocess_finish"}}},
    {E_DIST_SCORE_FINISH, "pdl_dist_score_finish", nullptr, {{NEED_AT_JOINED, "pdl_dist_score_finish without pdl_dist_score_begin"}}},
    {E_QUERY_SCORES, "pdl_query_scores", nullptr, {PDL_NEEDS_QUERY, {NEED_STREAM, nullptr}}},
    {E_QUERY_BATCH, "pdl_query_batch", nullptr, {PDL_NEEDS_QUERY, {NEED_STREAM, nullptr}}},
    {E_PLACE_QUERY, "pdl_place_query", "pdl_placement_of_edges", {PDL_NEEDS_QUERY, {NEED_NO_SHARD, nullptr}, {NEED_STREAM, nullptr}}},
    {E_PLACE_BATCH, "pdl_place_batch", "pdl_placement_batch_of_edges", {PDL_NEEDS_QUERY, {NEED_NO_SHARD, nullptr}, {NEED_STREAM, nullptr}}},
    {E_APPEND_GENOMES, "pdl_append_genomes", nullptr, {PDL_NEEDS_QUERY, {NEED_NO_SHARD, nullptr}, {NEED_STREAM, nullptr}}},
    {E_REMOVE_GENOMES, "pdl_remove_genomes", nullptr, {PDL_NEEDS_QUERY, {NEED_NO_SHARD, nullptr}, {NEED_STREAM, nullptr}}},
    {E_COMPUTE_FAMILIES, "pdl_compute_families", "pdl_families_of_edges", {PDL_NEEDS_QUERY, {NEED_NO_SHARD, nullptr}}},
};
#undef PDL_NEEDS_QUERY
static_assert(sizeof(PDL_GATE) / sizeof(PDL_GATE[0]) == E_COUNT, "one gate row per entry point");

inline bool pdl_meets(const pdl_ctx *c, Need need) {
    switch (need) {
    case NEED_INGESTED: return c->ingested;
    case NEED_BUILT: return c->preprocessed;
    case NEED_RANGES: return !c->only_complexity;
    case NEED_SINGLE_GPU: return !c->dist;
    case NEED_NO_SHARD: return !c->shard_set && c->dict_shard.empty();
    case NEED_STREAM: return c->keys_b.p && c->recpos.p && c->vals_b.p;
    case NEED_GENE_COSTS: return !(c->dist && c->dist_sender);
    case NEED_NO_DEAL: return c->dist_stage == DistStage::none;
    case NEED_AT_SLICE: return c->dist_stage == DistStage::slice_built;
    case NEED_ADOPTED: return c->dist_stage >= DistStage::adopted;
    case NEED_AT_JOINED: return c->dist_stage == DistStage::joined;
    case NEED_TUPLES: return c->dist_sender;
    case NEED_NO_TUPLES: return !c->dist_sender;
    case NEED_END: break;
    }
    return true;
}
// Throws the PDL_ERR_STATE refusal of the first need of the entry point's row the context does not meet; nothing of the context
// has been touched then.  (The row's edge_form: the entry point that does the same over gathered edges, where there is one.)
inline void require_state(const pdl_ctx *c, Entry entry) {
    const GateRow *row = PDL_GATE;
    while (row->entry != entry) row++;
    const char *who = row->who, *edge_form = row->edge_form;
    for (const GateNeed &n : row->needs) {
        if (n.need == NEED_END) return;
        if (pdl_meets(c, n.need)) continue;
        if (n.text) PDL_FAIL(PDL_ERR_STATE, "%s", n.text);
        switch (n.need) {
        case NEED_BUILT: PDL_FAIL(PDL_ERR_STATE, "%s before pdl_preprocess", who);
        case NEED_RANGES: PDL_FAIL(PDL_ERR_STATE, "%s: the context was preprocessed with only_complexity", who);
        case NEED_SINGLE_GPU:
            if (edge_form) PDL_FAIL(PDL_ERR_STATE, "%s: not available on a multi-GPU context (gather the edges: %s)", who, edge_form);
            PDL_FAIL(PDL_ERR_STATE, "%s: not available on a multi-GPU context", who);
        case NEED_NO_SHARD:
            if (edge_form) PDL_FAIL(PDL_ERR_STATE, "%s: a genome shard is in force, the context does not hold every genome's edges (gather them: %s)", who, edge_form);
            PDL_FAIL(PDL_ERR_STATE, "%s: not available with a genome shard in force", who);
        case NEED_STREAM: PDL_FAIL(PDL_ERR_STATE, "%s: the sorted k-mer stream was released (option low_memory)", who);
        default: PDL_FAIL(PDL_ERR_STATE, "%s: the context is not in the state the call needs", who);       // (no such row: every other need brings its text)
        }
    }
}
