// state_gate_check.cpp — the reset and the gate of pdl_state.h on every state a context can be in, as a program of its own so that
// it can be built with the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/state_gate_check.cpp -o state_gate_check && ./state_gate_check
//
// No device is touched and no HIP call is made: a pdl_ctx is only a struct here.  For every state below and every row of the gate
// the refusal's code and text are compared with what the entry points spelled inline before there was a table (`expected`: an if
// chain per entry point, its texts literals); every depth of pdl_stale must change exactly the members its table names; and no
// reset may leave a derived product (mirror, edges, families) valid on a context that is not scored — so that behind "a new set"
// they can only come back behind a scoring pass.
#include "../pandelos_amd/csrc/pdl_common.h"

#include <cstring>

void pdl_set_create_error(const std::string &) {}        // (guarded's, never reached here)

struct State {
    const char *name;
    bool ingested, built, only_complexity, shard, stream, scored, dist;
    int stage;            // 0 none | 1 slice built | 2 adopted | 3 joined | 4 scored
    bool sender;
};
static const State STATES[] = {
    //                                   ingested built  cplx   shard  stream scored dist   stage sender
    {"fresh",                            false,   false, false, false, false, false, false, 0, false},
    {"ingested",                         true,    false, false, false, false, false, false, 0, false},
    {"built",                            false,   true,  false, false, true,  false, false, 0, false},
    {"built from an ingest",             true,    true,  false, false, true,  false, false, 0, false},
    {"built with only_complexity",       false,   true,  true,  false, true,  false, false, 0, false},
    {"built under a shard",              false,   true,  false, true,  true,  false, false, 0, false},
    {"built, stream released",           false,   true,  false, false, false, false, false, 0, false},
    {"scored, edges and families valid", false,   true,  false, false, true,  true,  false, 0, false},
    {"multi-GPU, begun and failed",      false,   false, false, false, false, false, true,  0, false},
    {"multi-GPU, slice built",           false,   false, false, false, false, false, true,  1, false},
    {"multi-GPU, slice and tuples",      false,   false, false, false, false, false, true,  1, true},
    {"multi-GPU, adopted",               false,   true,  false, true,  false, false, true,  2, false},
    {"multi-GPU, adopted with tuples",   false,   true,  false, true,  false, false, true,  2, true},
    {"multi-GPU, joined",                false,   true,  false, true,  false, false, true,  3, false},
    {"multi-GPU, joined with tuples",    false,   true,  false, true,  false, false, true,  3, true},
    {"multi-GPU, scored",                false,   true,  false, true,  false, true,  true,  4, false},
    {"multi-GPU, scored with tuples",    false,   true,  false, true,  false, true,  true,  4, true},
};

static char g_dummy[3];
static void put(pdl_ctx &c, const State &s) {
    c.ingested = s.ingested; c.preprocessed = s.built; c.only_complexity = s.only_complexity;
    c.shard_set = s.shard;
    if (s.shard) { c.shard = {0, 2}; c.dict_shard = {0, 2}; } else { c.shard.clear(); c.dict_shard.clear(); }
    c.keys_b.p = s.stream ? &g_dummy[0] : nullptr; c.recpos.p = s.stream ? &g_dummy[1] : nullptr; c.vals_b.p = s.stream ? &g_dummy[2] : nullptr;
    c.scored = s.scored; c.mirror_valid = c.edges_valid = c.fam_valid = s.scored;
    c.tasks_ready = s.built;
    c.dist = s.dist; c.dist_stage = (DistStage) s.stage; c.dist_sender = s.sender;
    c.post_ext = s.stage >= 2 ? reinterpret_cast<uint2 *>(g_dummy) : nullptr;
}
static void unhook(pdl_ctx &c) { c.keys_b.p = c.recpos.p = c.vals_b.p = nullptr; }        // (nothing of g_dummy is the context's to free)

// What the entry point `e` answered in state `s` when its checks were spelled inline (nullptr: served as far as the state goes).
// pdl_genome_cost, pdl_sequence_costs and pdl_get_rank_table returned PDL_ERR_STATE without a text on an unbuilt context: theirs
// is the gate's "%s before pdl_preprocess".
static const char *expected(Entry e, const State &s) {
    const bool shard = s.shard, no_stream = !s.stream;
    switch (e) {
    case E_PREPROCESS_INGESTED: return s.ingested ? nullptr : "pdl_preprocess_ingested before pdl_ingest_faa";
    case E_GENOME_COST: return s.built ? nullptr : "pdl_genome_cost before pdl_preprocess";
    case E_SEQUENCE_COSTS:
        if (!s.built) return "pdl_sequence_costs before pdl_preprocess";
        if (s.dist && s.sender) return "per-gene costs are not kept by a multi-GPU build whose range lists came from the senders (pdl_genome_cost works)";
        return nullptr;
    case E_GET_RANK_TABLE: return s.built ? nullptr : "pdl_get_rank_table before pdl_preprocess";
    case E_GET_DICTIONARY:
        if (!s.built) return "pdl_get_dictionary before pdl_preprocess";
        if (s.dist) return "pdl_get_dictionary: a multi-GPU context keeps ranks only for its own interval";
        if (no_stream) return "pdl_get_dictionary: the sorted k-mer stream was released (option low_memory)";
        return nullptr;
    case E_SET_GENOME_SHARD: return s.dist && s.stage ? "genome shard: a multi-GPU build deals the genomes itself (pdl_dist_genome_owner)" : nullptr;
    case E_SCORE:         // (of a context that is not scored)
        if (!s.built) return "pdl_score_all before pdl_preprocess";
        if (s.only_complexity) return "the dictionary was built in complexity-only mode (no posting ranges)";
        if (s.dist) return "multi-GPU context: score with pdl_dist_score_begin / pdl_dist_score_finish";
        return nullptr;
    case E_DIST_FINISH:
        if (!s.dist || s.stage != 1) return "pdl_dist_preprocess_finish without pdl_dist_preprocess_begin";
        if (s.sender) return "pdl_dist_preprocess_finish after a pdl_dist_preprocess_ranges that built this run's range tuples (and took its group-head bits out): finish with pdl_dist_preprocess_finish_ranges";
        return nullptr;
    case E_DIST_RANGES:
        if (!s.dist || s.stage != 1) return "pdl_dist_preprocess_ranges without pdl_dist_preprocess_begin";
        if (s.sender) return "pdl_dist_preprocess_ranges has built this run's range tuples already (and took its group-head bits out): go on with pdl_dist_preprocess_finish_ranges";
        return nullptr;
    case E_DIST_FINISH_RANGES:
        return !s.dist || s.stage != 1 || !s.sender ? "pdl_dist_preprocess_finish_ranges without a pdl_dist_preprocess_ranges that said \"available\"" : nullptr;
    case E_DIST_GENOME_OWNER: return !s.dist || s.stage < 2 ? "pdl_dist_genome_owner before pdl_dist_preprocess_finish: the genomes have not been dealt" : nullptr;
    case E_DIST_SCORE_BEGIN: return !s.dist || s.stage < 2 ? "pdl_dist_score_begin before pdl_dist_preprocess_finish" : nullptr;
    case E_DIST_SCORE_FINISH: return !s.dist || s.stage != 3 ? "pdl_dist_score_finish without pdl_dist_score_begin" : nullptr;
    case E_QUERY_SCORES:
        if (!s.built) return "pdl_query_scores before pdl_preprocess";
        if (s.only_complexity) return "pdl_query_scores: the context was preprocessed with only_complexity";
        if (s.dist) return "pdl_query_scores: not available on a multi-GPU context";
        if (no_stream) return "pdl_query_scores: the sorted k-mer stream was released (option low_memory)";
        return nullptr;
    case E_QUERY_BATCH:
        if (!s.built) return "pdl_query_batch before pdl_preprocess";
        if (s.only_complexity) return "pdl_query_batch: the context was preprocessed with only_complexity";
        if (s.dist) return "pdl_query_batch: not available on a multi-GPU context";
        if (no_stream) return "pdl_query_batch: the sorted k-mer stream was released (option low_memory)";
        return nullptr;
    case E_PLACE_QUERY:
        if (!s.built) return "pdl_place_query before pdl_preprocess";
        if (s.only_complexity) return "pdl_place_query: the context was preprocessed with only_complexity";
        if (s.dist) return "pdl_place_query: not available on a multi-GPU context (gather the edges: pdl_placement_of_edges)";
        if (shard) return "pdl_place_query: a genome shard is in force, the context does not hold every genome's edges (gather them: pdl_placement_of_edges)";
        if (no_stream) return "pdl_place_query: the sorted k-mer stream was released (option low_memory)";
        return nullptr;
    case E_PLACE_BATCH:
        if (!s.built) return "pdl_place_batch before pdl_preprocess";
        if (s.only_complexity) return "pdl_place_batch: the context was preprocessed with only_complexity";
        if (s.dist) return "pdl_place_batch: not available on a multi-GPU context (gather the edges: pdl_placement_batch_of_edges)";
        if (shard) return "pdl_place_batch: a genome shard is in force, the context does not hold every genome's edges (gather them: pdl_placement_batch_of_edges)";
        if (no_stream) return "pdl_place_batch: the sorted k-mer stream was released (option low_memory)";
        return nullptr;
    case E_APPEND_GENOMES:
        if (!s.built) return "pdl_append_genomes before pdl_preprocess";
        if (s.only_complexity) return "pdl_append_genomes: the context was preprocessed with only_complexity";
        if (s.dist) return "pdl_append_genomes: not available on a multi-GPU context";
        if (shard) return "pdl_append_genomes: not available with a genome shard in force";
        if (no_stream) return "pdl_append_genomes: the sorted k-mer stream was released (option low_memory)";
        return nullptr;
    case E_REMOVE_GENOMES:
        if (!s.built) return "pdl_remove_genomes before pdl_preprocess";
        if (s.only_complexity) return "pdl_remove_genomes: the context was preprocessed with only_complexity";
        if (s.dist) return "pdl_remove_genomes: not available on a multi-GPU context";
        if (shard) return "pdl_remove_genomes: not available with a genome shard in force";
        if (no_stream) return "pdl_remove_genomes: the sorted k-mer stream was released (option low_memory)";
        return nullptr;
    case E_COMPUTE_FAMILIES:
        if (!s.built) return "pdl_compute_families before pdl_preprocess";
        if (s.only_complexity) return "pdl_compute_families: the context was preprocessed with only_complexity";
        if (s.dist) return "pdl_compute_families: not available on a multi-GPU context (gather the edges: pdl_families_of_edges)";
        if (shard) return "pdl_compute_families: a genome shard is in force, the context does not hold every genome's edges (gather them: pdl_families_of_edges)";
        return nullptr;
    case E_COUNT: break;
    }
    return "?";
}

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); failures++; } } while (0)

static int check_gate(pdl_ctx &c) {
    int cells = 0;
    for (const State &s : STATES)
        for (int e = 0; e < E_COUNT; e++) {
            if (e == E_SCORE && s.scored) continue;          // (a scored context is served without being asked)
            put(c, s);
            const char *want = expected((Entry) e, s);
            int code = PDL_OK;
            std::string msg;
            try { require_state(&c, (Entry) e); } catch (const pdl_error &err) { code = err.code; msg = err.msg; }
            CHECK(code == (want ? PDL_ERR_STATE : PDL_OK) && msg == (want ? want : ""), "%s / %s: code %d \"%s\", expected \"%s\"", PDL_GATE[e].who, s.name, code,
                  msg.c_str(), want ? want : "(served)");
            cells++;
        }
    return cells;
}

// the members pdl_stale may touch, and a few it must not
struct Words {          // (64-bit words all: no padding, so that two of them compare as bytes)
    uint64_t preprocessed, tasks_ready, reshard_pending, scored, mirror, edges, fam, plans, dist, sender, shard_set, ingested, only_complexity, layout_deferred,
             short_valid, U, Ushared, NG, P, M, R, N, G, stage, post_ext, shard, dict_shard;
    bool operator==(const Words &o) const { return !memcmp(this, &o, sizeof(*this)); }
};
static Words read(const pdl_ctx &c) {
    Words w;
    memset(&w, 0, sizeof(w));
    w.preprocessed = c.preprocessed; w.tasks_ready = c.tasks_ready; w.reshard_pending = c.reshard_pending; w.scored = c.scored;
    w.mirror = c.mirror_valid; w.edges = c.edges_valid; w.fam = c.fam_valid;
    w.plans = c.qb.hbm_cols == 7 && c.qbb.stage.bytes == 7 && c.pb.base_serial == 7;
    w.dist = c.dist; w.sender = c.dist_sender; w.shard_set = c.shard_set; w.ingested = c.ingested; w.only_complexity = c.only_complexity;
    w.layout_deferred = c.layout_deferred; w.short_valid = c.short_valid;
    w.U = c.U; w.Ushared = c.Ushared; w.NG = c.NG; w.P = c.P; w.M = c.M; w.R = c.R; w.N = c.N; w.G = c.G;
    w.stage = (uint64_t) c.dist_stage; w.post_ext = (uint64_t) (uintptr_t) c.post_ext; w.shard = c.shard.size(); w.dict_shard = c.dict_shard.size();
    return w;
}
static void check_reset(pdl_ctx &c) {
    for (const State &s : STATES)
        for (Stale depth : {Stale::set, Stale::build, Stale::scores_and_tasks, Stale::scores}) {
            put(c, s);
            // everything a reset can drop is up, whatever the state, so that a member it should have left alone shows
            c.tasks_ready = c.reshard_pending = c.mirror_valid = c.edges_valid = c.fam_valid = true;
            c.qb.hbm_cols = 7; c.qbb.stage.bytes = 7; c.pb.base_serial = 7;
            c.U = 11; c.Ushared = 12; c.NG = 13; c.P = 14; c.M = 15; c.R = 16; c.N = 17; c.G = 4;
            c.layout_deferred = true; c.short_valid = true;
            Words want = read(c);
            want.scored = want.mirror = want.edges = want.fam = false;
            if (depth != Stale::scores) want.tasks_ready = false;
            if (depth == Stale::set || depth == Stale::build) want.preprocessed = want.reshard_pending = false;
            if (depth == Stale::set) {
                want.plans = false;
                want.U = want.Ushared = want.NG = want.P = want.M = 0;
                if (s.dist) { want.shard_set = false; want.shard = 0; }       // (the deal of a multi-GPU build; a caller's shard stays)
                want.dist = want.sender = false; want.stage = 0; want.post_ext = 0;
            }
            pdl_stale(&c, depth);
            const Words got = read(c);
            CHECK(got == want, "pdl_stale, depth %d on \"%s\": other members changed than the table names", (int) depth, s.name);
            CHECK(got.scored || !(got.mirror || got.edges || got.fam), "pdl_stale, depth %d on \"%s\": a derived product is valid on a context that is not scored", (int) depth, s.name);
            c.qbb.stage.bytes = 0;
        }
}

int main() {
    for (int e = 0; e < E_COUNT; e++) CHECK(PDL_GATE[e].entry == (Entry) e, "row %d of the gate is entry %d's", e, (int) PDL_GATE[e].entry);
    pdl_ctx *c = new pdl_ctx();
    const int cells = check_gate(*c);
    check_reset(*c);
    unhook(*c);
    delete c;
    printf("%d cells of the gate, %zu states x 4 depths of the reset, %d failures\n", cells, sizeof(STATES) / sizeof(STATES[0]), failures);
    return failures ? 1 : 0;
}
