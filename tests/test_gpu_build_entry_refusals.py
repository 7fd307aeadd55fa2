"""Which build, score and multi-GPU entry point refuses which state of the context — through the C ABI, with stale bytes in
every output first — and in which order a build with several things wrong reports them.

The table (pdl_state.h keeps it at the gate every entry point calls; test_gpu_entry_refusals.py runs the incremental rows):

    entry point                         needs
    pdl_preprocess_ingested             ingested
    pdl_genome_cost, pdl_get_rank_table built
    pdl_sequence_costs                  built, per-gene costs kept (no sender-built tuples)
    pdl_get_dictionary                  built, single-GPU, stream held
    pdl_set_genome_shard                no multi-GPU build begun
    pdl_score_all, pdl_scores_counts,
      pdl_compute_scores, _edges        built, ranges, single-GPU — unless the context is scored: then they are served
    pdl_dist_preprocess_finish, _ranges multi-GPU build at "slice built", tuples not built
    pdl_dist_preprocess_finish_ranges   multi-GPU build at "slice built", tuples built
    pdl_dist_genome_owner, _score_begin multi-GPU build at "adopted" or later
    pdl_dist_score_finish               multi-GPU build at "joined"

Every state below meets every row; where ``expected`` says the state refuses the call it is made: the code, the exact message
(literals, as the entry points spelled them before there was a table), the outputs zeroed where the entry point zeroes them
(pdl_compute_scores, pdl_compute_edges) and untouched everywhere else.  Then every built context still gives the CPU oracle's
cost and Scores blocks."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests.test_gpu_dist_protocol import Ranks

pytestmark = pytest.mark.gpu

K = 3
STALE = 0xA5
NAME = "entry_refusals_4x12"


@pytest.fixture(scope="module")
def gene_set():
    from pandelos_amd.synth import make_gene_set
    return make_gene_set(genomes=4, genes_per_genome=12, mean_len=40, sub_rate=0.1, seed=11)


@pytest.fixture(scope="module")
def oracle(gene_set):
    from oracle import binding as ob
    gs = gene_set
    return ob.Oracle(gs.residues, gs.offsets, gs.genome_of, K)


@pytest.fixture(scope="module")
def sets(gene_set):
    """The set as tests.test_gpu_dist_protocol.Ranks takes it (no fixture file: the oracle is the reference here)."""
    import torch
    gs = gene_set
    dev = torch.device("cuda", 0)
    t_res = torch.from_numpy(np.concatenate([gs.residues, np.zeros((-len(gs.residues)) % 16 + 16, np.uint8)])).to(dev)
    t_off = torch.from_numpy(gs.offsets.astype(np.int64)).to(dev)
    t_gen = torch.from_numpy(gs.genome_of.astype(np.int32)).to(dev)
    return {NAME: (gs.residues, gs.offsets.astype(np.uint64), gs.genome_of.astype(np.uint32), K, {"genomes": gs.genomes}, (t_res, t_off, t_gen))}


def _stale(ctype, count=1):
    a = (ctype * count)()
    C.memset(a, STALE, C.sizeof(a))
    return a


def _state(ingested=False, built=False, cplx=False, shard=False, stream=False, scored=False, dist=False, stage=0, sender=False):
    return dict(ingested=ingested, built=built, cplx=cplx, shard=shard, stream=stream, scored=scored, dist=dist, stage=stage, sender=sender)


SCORE_ENTRIES = ("pdl_score_all", "pdl_scores_counts", "pdl_compute_scores", "pdl_compute_edges")
BARE = ("pdl_genome_cost", "pdl_sequence_costs", "pdl_get_rank_table")     # returned PDL_ERR_STATE without a text before the gate
ENTRIES = ("pdl_preprocess_ingested",) + SCORE_ENTRIES + BARE + (
    "pdl_get_dictionary", "pdl_set_genome_shard", "pdl_dist_preprocess_finish", "pdl_dist_preprocess_ranges",
    "pdl_dist_preprocess_finish_ranges", "pdl_dist_genome_owner", "pdl_dist_score_begin", "pdl_dist_score_finish")


def expected(entry, s):
    """-> the message of the PDL_ERR_STATE refusal, or None where the state serves the call."""
    if entry == "pdl_preprocess_ingested":
        return None if s["ingested"] else "pdl_preprocess_ingested before pdl_ingest_faa"
    if entry in SCORE_ENTRIES:
        if s["scored"]:
            return None
        if not s["built"]:
            return "pdl_score_all before pdl_preprocess"
        if s["cplx"]:
            return "the dictionary was built in complexity-only mode (no posting ranges)"
        return "multi-GPU context: score with pdl_dist_score_begin / pdl_dist_score_finish" if s["dist"] else None
    if entry in ("pdl_genome_cost", "pdl_get_rank_table"):
        return None if s["built"] else f"{entry} before pdl_preprocess"
    if entry == "pdl_sequence_costs":
        if not s["built"]:
            return "pdl_sequence_costs before pdl_preprocess"
        if s["dist"] and s["sender"]:
            return "per-gene costs are not kept by a multi-GPU build whose range lists came from the senders (pdl_genome_cost works)"
        return None
    if entry == "pdl_get_dictionary":
        if not s["built"]:
            return "pdl_get_dictionary before pdl_preprocess"
        if s["dist"]:
            return "pdl_get_dictionary: a multi-GPU context keeps ranks only for its own interval"
        return None if s["stream"] else "pdl_get_dictionary: the sorted k-mer stream was released (option low_memory)"
    if entry == "pdl_set_genome_shard":
        return "genome shard: a multi-GPU build deals the genomes itself (pdl_dist_genome_owner)" if s["dist"] and s["stage"] else None
    at_slice = s["dist"] and s["stage"] == 1
    if entry == "pdl_dist_preprocess_finish":
        if not at_slice:
            return "pdl_dist_preprocess_finish without pdl_dist_preprocess_begin"
        return ("pdl_dist_preprocess_finish after a pdl_dist_preprocess_ranges that built this run's range tuples (and took its group-head bits out): "
                "finish with pdl_dist_preprocess_finish_ranges") if s["sender"] else None
    if entry == "pdl_dist_preprocess_ranges":
        if not at_slice:
            return "pdl_dist_preprocess_ranges without pdl_dist_preprocess_begin"
        return ("pdl_dist_preprocess_ranges has built this run's range tuples already (and took its group-head bits out): "
                "go on with pdl_dist_preprocess_finish_ranges") if s["sender"] else None
    if entry == "pdl_dist_preprocess_finish_ranges":
        return None if at_slice and s["sender"] else 'pdl_dist_preprocess_finish_ranges without a pdl_dist_preprocess_ranges that said "available"'
    adopted = s["dist"] and s["stage"] >= 2
    if entry == "pdl_dist_genome_owner":
        return None if adopted else "pdl_dist_genome_owner before pdl_dist_preprocess_finish: the genomes have not been dealt"
    if entry == "pdl_dist_score_begin":
        return None if adopted else "pdl_dist_score_begin before pdl_dist_preprocess_finish"
    assert entry == "pdl_dist_score_finish"
    return None if s["dist"] and s["stage"] == 3 else "pdl_dist_score_finish without pdl_dist_score_begin"


def _refusal(nat, entry, gs, dummy):
    """One call that the state must refuse -> (return code, message).  The arguments are well-formed as far as a call can tell
    before it looks at the state (``dummy``: aligned device memory nothing may get as far as reading); asserts what became of
    the outputs."""
    from pandelos_amd import _lib
    lib, ctx = nat._lib, nat._ctx
    G, N = gs.genomes, gs.genes
    zeroed, kept = [], []
    zeros = np.zeros(max(G, 3), np.uint64)
    if entry == "pdl_preprocess_ingested":
        cost = _stale(_lib.PdlCost)
        rc = lib.pdl_preprocess_ingested(ctx, K, 0, cost)
        kept = [cost]
    elif entry == "pdl_score_all":
        rc = lib.pdl_score_all(ctx)
    elif entry == "pdl_scores_counts":
        out = _stale(C.c_uint32, G)
        rc = lib.pdl_scores_counts(ctx, out)
        kept = [out]
    elif entry == "pdl_compute_scores":
        out = _stale(_lib.PdlScores)
        rc = lib.pdl_compute_scores(ctx, 0, out)
        zeroed = [out]
    elif entry == "pdl_compute_edges":
        out = _stale(_lib.PdlEdges)
        rc = lib.pdl_compute_edges(ctx, 0, out)
        zeroed = [out]
    elif entry == "pdl_genome_cost":
        out = _stale(C.c_uint64)
        rc = lib.pdl_genome_cost(ctx, 0, out)
        kept = [out]
    elif entry == "pdl_sequence_costs":
        cost, kseq = _stale(C.c_uint64, N), _stale(C.c_uint32, N)
        rc = lib.pdl_sequence_costs(ctx, cost, kseq)
        kept = [cost, kseq]
    elif entry == "pdl_get_rank_table":
        table, lm = _stale(C.c_uint8, 256), _stale(C.c_uint64)
        rc = lib.pdl_get_rank_table(ctx, table, lm)
        kept = [table, lm]
    elif entry == "pdl_get_dictionary":
        u = 1 << 14
        ranks, seqs, counts = _stale(C.c_uint64, u), _stale(C.c_uint32, u), _stale(C.c_uint32, u)
        rc = lib.pdl_get_dictionary(ctx, ranks, seqs, counts)
        kept = [ranks, seqs, counts]
    elif entry == "pdl_set_genome_shard":
        rc = lib.pdl_set_genome_shard(ctx, np.array([0], np.uint32).ctypes.data, 1)
    elif entry == "pdl_dist_preprocess_finish":
        cost = _stale(_lib.PdlCost)
        rc = lib.pdl_dist_preprocess_finish(ctx, dummy.data_ptr(), 1, zeros.ctypes.data, cost)
        kept = [cost]
    elif entry == "pdl_dist_preprocess_ranges":
        out = _stale(_lib.PdlDistRanges)
        rc = lib.pdl_dist_preprocess_ranges(ctx, np.ones(2, np.uint64).ctypes.data, zeros.ctypes.data, zeros.ctypes.data, out)
        kept = [out]
    elif entry == "pdl_dist_preprocess_finish_ranges":
        cost = _stale(_lib.PdlCost)
        rc = lib.pdl_dist_preprocess_finish_ranges(ctx, dummy.data_ptr(), 1, None, None, 0, zeros.ctypes.data, cost)
        kept = [cost]
    elif entry == "pdl_dist_genome_owner":
        out = _stale(C.c_uint32, G)
        rc = lib.pdl_dist_genome_owner(ctx, out)
        kept = [out]
    elif entry == "pdl_dist_score_begin":
        out = _stale(_lib.PdlDistOutbox)
        rc = lib.pdl_dist_score_begin(ctx, out)
        kept = [out]
    else:
        assert entry == "pdl_dist_score_finish"
        rc = lib.pdl_dist_score_finish(ctx, dummy.data_ptr(), 0)
    assert rc != _lib.PDL_OK, f"{entry}: the call was served"
    for s in zeroed:
        assert bytes(s) == bytes(C.sizeof(s)), f"{entry}: {type(s).__name__} is not zeroed after a refusal"
    for s in kept:
        assert bytes(s) == bytes([STALE]) * C.sizeof(s), f"{entry}: {type(s).__name__} was written by a refusal"
    return rc, lib.pdl_last_error(ctx).decode()


def _single_contexts(gs, faa):
    """name -> (context, its state): every state a single-GPU context can refuse one of the entry points in."""
    from pandelos_amd.pangene_native import PangeneNative
    gs.write_faa(faa)
    out = {"fresh": (PangeneNative.open(), _state())}
    ingested = PangeneNative.open()
    ingested.ingest_faa(faa)
    out["ingested"] = (ingested, _state(ingested=True))
    out["built"] = (PangeneNative.from_arrays(K, gs.residues, gs.offsets, gs.genome_of), _state(built=True, stream=True))
    out["built with only_complexity"] = (PangeneNative.from_arrays(K, gs.residues, gs.offsets, gs.genome_of, only_complexity=True),
                                         _state(built=True, cplx=True, stream=True))
    shard = PangeneNative.open()
    shard.set_genome_shard([0, 2])
    shard.preprocess(K, gs.residues, gs.offsets, gs.genome_of)
    out["built under a shard"] = (shard, _state(built=True, shard=True, stream=True))
    low = PangeneNative.open()
    low.set_option("low_memory", 1)
    low.preprocess(K, gs.residues, gs.offsets, gs.genome_of)
    out["built, stream released"] = (low, _state(built=True))
    scored = PangeneNative.from_arrays(K, gs.residues, gs.offsets, gs.genome_of)
    scored.generate_families()                                            # scored, and the edges and the families are valid
    out["scored, edges and families valid"] = (scored, _state(built=True, stream=True, scored=True))
    return out


# multi-GPU: how a fresh Ranks gets to a stage -> (stage, tuples built)
def _begun(rk):
    rk.begin()
    return 1, False


def _ranged(rk):
    rk.begin()
    assert rk.ranges(), "this set takes the senders' flow over these ranks"
    return 1, True


def _finished_by_owners(rk):
    assert not rk.build(sender=False)
    return 2, False


def _finished_by_senders(rk):
    assert rk.build(), "this set takes the senders' flow over these ranks"
    return 2, True


def _joined(rk):
    _finished_by_senders(rk)
    rk.score_begin()
    return 3, True


def _scored(rk):
    _finished_by_senders(rk)
    rk.score()
    return 4, True


def _scored_by_owners(rk):
    _finished_by_owners(rk)
    rk.score()
    return 4, False


DIST_STATES = {"slice built": _begun, "slice built, tuples built": _ranged, "adopted": _finished_by_owners, "adopted, tuples built": _finished_by_senders,
               "joined, tuples built": _joined, "scored, tuples built": _scored, "scored": _scored_by_owners}
ONE_RANK = ("slice built", "adopted", "scored")


def _assert_oracle(nat_of_genome, genomes, ora, label):
    for g in genomes:
        H.assert_scores_equal(nat_of_genome(g).generate_scores_part(g).as_dict(), ora.scores(g), f"{label}: genome {g} after the refusals")


def test_every_state_refuses_what_the_table_says(gene_set, oracle, sets, tmp_path):
    import torch
    from pandelos_amd import _lib
    gs = gene_set
    dummy = torch.zeros(16, dtype=torch.int64, device=torch.device("cuda", 0))
    singles = _single_contexts(gs, tmp_path / "set.faa")
    ranks = {}
    made = 0

    def run(label, nat, state):
        nonlocal made
        for entry in ENTRIES:
            want = expected(entry, state)
            if want is None:
                continue
            rc, msg = _refusal(nat, entry, gs, dummy)
            print(f"{entry} / {label}: rc={rc} {msg!r}")
            assert rc == _lib.PDL_ERR_STATE, (entry, label, rc, msg)
            # NEW WITH THE GATE where `entry in BARE and not state["built"]` — the one assertion of this file (with its like in the
            # test below) that the library before the gate does not pass: these three returned the bare code and left the text of
            # some earlier failure in pdl_last_error
            assert msg == want, (entry, label, msg)
            made += 1

    try:
        for label, (nat, state) in singles.items():
            run(label, nat, state)
        for world in (1, 2):
            for label, reach in DIST_STATES.items():
                if world == 1 and label not in ONE_RANK:
                    continue
                rk = ranks[(world, label)] = Ranks(sets, NAME, world)
                stage, sender = reach(rk)
                for r, nat in enumerate(rk.nats):
                    run(f"{label}, rank {r} of {world}", nat, _state(built=stage >= 2, shard=True, scored=stage == 4, dist=True, stage=stage, sender=sender))
        print(f"{made} refusals")
        assert made >= 200          # (8 single-GPU and 17 multi-GPU contexts, sixteen entry points)

        # ---- the aftermath: what was built is still what the oracle says -------------------------------------------------------
        for label, (nat, state) in singles.items():
            if state["built"]:
                if not state["shard"]:                                    # (under a shard "Total cost" is the lookups of the shard's genes)
                    assert nat.cost.total_cost == oracle.total_cost, label
                if not state["cplx"]:
                    _assert_oracle(lambda g: nat, (0, 2) if state["shard"] else range(gs.genomes), oracle, label)
        for (world, label), rk in ranks.items():
            stage = DIST_STATES[label].__name__
            if stage in ("_begun", "_ranged"):
                continue
            if stage == "_joined":
                rk.exchange_cells()
                rk.score_finish()
            elif not stage.startswith("_scored"):
                rk.score()
            owner = rk.nats[0].dist_genome_owner()
            assert sum(int(n.cost.total_cost) for n in rk.nats) == oracle.total_cost, (world, label)
            _assert_oracle(lambda g: rk.nats[int(owner[g])], range(gs.genomes), oracle, f"{label}, {world} ranks")
    finally:
        for nat, _ in singles.values():
            nat.close()
        for rk in ranks.values():
            rk.close()


def test_a_genome_out_of_range_is_an_argument_refusal_that_names_pdl_genome_cost(gene_set):
    from pandelos_amd import _lib
    from pandelos_amd.pangene_native import PangeneNative
    gs = gene_set
    nat = PangeneNative.from_arrays(K, gs.residues, gs.offsets, gs.genome_of)
    try:
        out = _stale(C.c_uint64)
        assert nat._lib.pdl_genome_cost(nat._ctx, gs.genomes, out) == _lib.PDL_ERR_ARGUMENT
        assert bytes(out) == bytes([STALE]) * 8
        # NEW WITH THE GATE, as above: the bare code has a text now
        assert nat._lib.pdl_last_error(nat._ctx).decode() == f"pdl_genome_cost: genome {gs.genomes} out of range ({gs.genomes} genomes)"
    finally:
        nat.close()


# ---- the order in which a build with several things wrong reports them -----------------------------------------------------------
# pointers and alignment, offsets[0] (the span, for device input), then — behind the reset: a build refused from here on leaves a
# context that refuses every reader — k, then n, then the genome layout
def _is_built(nat):
    out = _stale(C.c_uint64)
    return nat._lib.pdl_genome_cost(nat._ctx, 0, out) == 0


def _build_call(nat, entry, gs, t, *, res=True, off=True, gen=True, n=None, n_res=None, k=K, world=1, rank=0, misaligned=False, off0=0, sparse_ids=False):
    """-> (code, message, built afterwards) of one build call; the keywords make single arguments wrong."""
    from pandelos_amd import _lib
    lib, ctx = nat._lib, nat._ctx
    n = gs.genes if n is None else n
    n_res = len(gs.residues) if n_res is None else n_res
    cost = _stale(_lib.PdlCost)
    if entry == "pdl_preprocess":
        offsets = gs.offsets.astype(np.uint64).copy()
        offsets[0] = off0
        ids = gs.genome_of.astype(np.uint32).copy()
        if sparse_ids:
            ids[-1] = 1000
        rc = lib.pdl_preprocess(ctx, gs.residues.ctypes.data if res else None, offsets.ctypes.data if off else None, ids.ctypes.data if gen else None, n, k, 0, cost)
    elif entry == "pdl_preprocess_ingested":
        rc = lib.pdl_preprocess_ingested(ctx, k, 0, cost)
    else:
        t_res, t_off, t_gen = t
        p_res = (t_res.data_ptr() + (1 if misaligned else 0)) if res else None
        if entry == "pdl_preprocess_device":
            rc = lib.pdl_preprocess_device(ctx, p_res, t_off.data_ptr() if off else None, t_gen.data_ptr() if gen else None, n, n_res, k, 0, cost)
        else:
            assert entry == "pdl_dist_preprocess_begin"
            rc = lib.pdl_dist_preprocess_begin(ctx, p_res, t_off.data_ptr() if off else None, t_gen.data_ptr() if gen else None, n, n_res, k, world, rank,
                                               C.byref(_lib.PdlDistSlice()))
    assert rc != 0, f"{entry}: the call was served"
    assert bytes(cost) == bytes([STALE]) * C.sizeof(cost), f"{entry}: pdl_cost was written by a refused build"
    return rc, lib.pdl_last_error(ctx).decode(), _is_built(nat)


def test_a_build_with_several_things_wrong_reports_them_in_order(gene_set, oracle, sets, tmp_path):
    from pandelos_amd import _lib
    from pandelos_amd.pangene_native import PangeneNative
    gs = gene_set
    t = sets[NAME][5]
    R = len(gs.residues)
    ARG, KV, EMPTY, STATE = _lib.PDL_ERR_ARGUMENT, _lib.PDL_ERR_KVALUE, _lib.PDL_ERR_EMPTY, _lib.PDL_ERR_STATE
    span = f"offsets[0] = 0, offsets[n] = {R} do not span the {R + 1} residues"
    # entry point -> [(what is wrong, code, message, the context is still built behind the refusal)], first-reported first
    cases = {
        "pdl_preprocess": [
            (dict(gen=False, off0=1, k=0, sparse_ids=True), ARG, "null input pointer", True),
            (dict(off0=1, k=0, sparse_ids=True), ARG, "offsets[0] must be 0", True),
            (dict(k=0, n=0, sparse_ids=True), KV, "K value must be greater than 0.", False),
            (dict(n=0, sparse_ids=True), EMPTY, "empty dataset", False),
            (dict(sparse_ids=True), ARG, f"genome ids are not dense: max id 1000 with {gs.genes} genes", False),
        ],
        "pdl_preprocess_device": [
            (dict(off=False, misaligned=True, n_res=R + 1, k=0), ARG, "null input pointer", True),
            (dict(misaligned=True, n_res=R + 1, k=0), ARG, "d_residues must be 16-byte aligned", True),
            (dict(n_res=R + 1, k=0), ARG, span, True),
            (dict(k=0, n=0), KV, "K value must be greater than 0.", False),
            (dict(n=0), EMPTY, "empty dataset", False),
        ],
        "pdl_dist_preprocess_begin": [
            (dict(off=False, misaligned=True, world=2, rank=2, n_res=R + 1, k=0), ARG, "null input pointer", True),
            (dict(misaligned=True, world=2, rank=2, n_res=R + 1, k=0), ARG, "d_residues must be 16-byte aligned", True),
            (dict(world=2, rank=2, n_res=R + 1, k=0), ARG, "rank 2 of 2 (at most 64 ranks)", True),
            (dict(n_res=R + 1, k=0), ARG, span, False),          # (the reset is in front of the read of the offsets' ends)
            (dict(k=0, n=0), KV, "K value must be greater than 0.", False),
            (dict(n=0), EMPTY, "empty dataset", False),
        ],
    }
    nat = PangeneNative.open()
    try:
        for entry, rows in cases.items():
            for wrong, code, text, stays_built in rows:
                nat.preprocess(K, gs.residues, gs.offsets, gs.genome_of)
                rc, msg, built = _build_call(nat, entry, gs, t, **wrong)
                print(f"{entry} {wrong}: rc={rc} {msg!r} built={built}")
                assert (rc, msg, built) == (code, text, stays_built), (entry, wrong, rc, msg, built)
        # pdl_preprocess_ingested: the state first, then k
        rc, msg, _ = _build_call(nat, "pdl_preprocess_ingested", gs, t, k=0)
        assert (rc, msg) == (STATE, "pdl_preprocess_ingested before pdl_ingest_faa"), (rc, msg)
        gs.write_faa(tmp_path / "set.faa")
        nat.ingest_faa(tmp_path / "set.faa")
        rc, msg, built = _build_call(nat, "pdl_preprocess_ingested", gs, t, k=0)
        assert (rc, msg, built) == (KV, "K value must be greater than 0.", False), (rc, msg, built)
        # ... and the context builds and scores the set behind all of it
        nat.preprocess_ingested(K)
        assert nat.cost.total_cost == oracle.total_cost
        _assert_oracle(lambda g: nat, range(gs.genomes), oracle, "behind the refused builds")
    finally:
        nat.close()
