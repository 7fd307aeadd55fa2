"""Which incremental entry point refuses which state of the context, and the argument checks on new genes that four of them
share — through the C ABI, with stale bytes in every output first.

The table (pdl_state.h keeps it, with the other entry points' rows, at the gate the six entry points call):

    entry point            built  ranges  single-GPU  no shard  stream held
    pdl_query_scores        yes    yes      yes         -          yes
    pdl_query_batch         yes    yes      yes         -          yes
    pdl_place_query         yes    yes      yes        yes         yes
    pdl_append_genomes      yes    yes      yes        yes         yes
    pdl_remove_genomes      yes    yes      yes        yes         yes
    pdl_compute_families    yes    yes      yes        yes          -

Every "yes" cell is run here: PDL_ERR_STATE, a message that names the entry point, outputs all-zero bytes.  The "-" cells (a
query under a genome shard, families after low_memory) are served, not refused; other suites run the first, none the second.
pdl_cost is an output of a successful append / removal only: a refusal leaves the caller's bytes as they were."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

K = 3
STALE = 0xA5
COLUMNS = ("built", "ranges", "single-GPU", "no shard", "stream held")
TABLE = {
    "pdl_query_scores": (1, 1, 1, 0, 1),
    "pdl_query_batch": (1, 1, 1, 0, 1),
    "pdl_place_query": (1, 1, 1, 1, 1),
    "pdl_append_genomes": (1, 1, 1, 1, 1),
    "pdl_remove_genomes": (1, 1, 1, 1, 1),
    "pdl_compute_families": (1, 1, 1, 1, 0),
}
GENE_ENTRIES = ("pdl_query_scores", "pdl_query_batch", "pdl_place_query", "pdl_append_genomes")


@pytest.fixture(scope="module")
def gene_set():
    from pandelos_amd.synth import make_gene_set
    return make_gene_set(genomes=4, genes_per_genome=12, mean_len=40, sub_rate=0.1, seed=11)


def _new_genes(gs):
    """Genes of the set's last genome again: valid arguments for every entry point that takes genes."""
    ids = np.nonzero(gs.genome_of == gs.genomes - 1)[0]
    lo, hi = int(gs.offsets[ids[0]]), int(gs.offsets[ids[-1] + 1])
    return gs.residues[lo:hi].copy(), (gs.offsets[ids[0]:ids[-1] + 2] - np.uint64(lo)).astype(np.uint64)


def _stale(ctype, count=1):
    a = (ctype * count)()
    C.memset(a, STALE, C.sizeof(a))
    return a


def _call(nat, entry, res, off, n, null_res=False):
    """-> (return code, message); asserts on a failure that the outputs are zero (and the cost of an append / removal untouched)."""
    from pandelos_amd import _lib
    lib, ctx = nat._lib, nat._ctx
    p_res = None if null_res or res is None else res.ctypes.data
    p_off = None if off is None else off.ctypes.data
    zeroed, kept = [], []
    if entry == "pdl_query_scores":
        out, info = _stale(_lib.PdlScores), _stale(_lib.PdlQueryInfo)
        rc = lib.pdl_query_scores(ctx, p_res, p_off, n, out, info)
        zeroed = [out, info]
    elif entry == "pdl_query_batch":
        out, info, binfo = _stale(_lib.PdlScores), _stale(_lib.PdlQueryInfo), _stale(_lib.PdlQueryBatchInfo)
        begin = np.array([0, n], np.uint32)
        rc = lib.pdl_query_batch(ctx, p_res, p_off, begin.ctypes.data, n, 1, out, info, binfo)
        zeroed = [out, info, binfo]
    elif entry == "pdl_place_query":
        out, info = _stale(_lib.PdlPlacement), _stale(_lib.PdlQueryInfo)
        rc = lib.pdl_place_query(ctx, p_res, p_off, n, out, info)
        zeroed = [out, info]
    elif entry == "pdl_append_genomes":
        cost, info = _stale(_lib.PdlCost), _stale(_lib.PdlAppendInfo)
        rc = lib.pdl_append_genomes(ctx, p_res, p_off, None, n, cost, info)
        zeroed, kept = [info], [cost]
    elif entry == "pdl_remove_genomes":
        cost, info = _stale(_lib.PdlCost), _stale(_lib.PdlRemoveInfo)
        ids = np.array([0], np.uint32)
        rc = lib.pdl_remove_genomes(ctx, ids.ctypes.data, 1, cost, info)
        zeroed, kept = [info], [cost]
    else:
        assert entry == "pdl_compute_families"
        out = _stale(_lib.PdlFamilies)
        rc = lib.pdl_compute_families(ctx, out)
        zeroed = [out]
    assert rc != _lib.PDL_OK, f"{entry}: the call was served"
    for s in zeroed:
        assert bytes(s) == bytes(C.sizeof(s)), f"{entry}: {type(s).__name__} is not zeroed after a refusal"
    for s in kept:
        assert bytes(s) == bytes([STALE]) * C.sizeof(s), f"{entry}: {type(s).__name__} was written by a refusal"
    return rc, lib.pdl_last_error(ctx).decode()


def _contexts(gs):
    """One context per column of the table: the state that column's "yes" refuses."""
    import torch
    from pandelos_amd.pangene_native import PangeneNative
    fresh = PangeneNative.open()
    cplx = PangeneNative.from_arrays(K, gs.residues, gs.offsets, gs.genome_of, only_complexity=True)
    dist = PangeneNative.open()                                           # a one-rank multi-GPU context
    dev = torch.device("cuda", 0)
    t_res = torch.from_numpy(np.concatenate([gs.residues, np.zeros(32, np.uint8)])).to(dev)
    t_off = torch.from_numpy(gs.offsets.astype(np.int64)).to(dev)
    t_gen = torch.from_numpy(gs.genome_of.astype(np.int32)).to(dev)
    dist.dist_preprocess_begin(K, t_res.data_ptr(), t_off.data_ptr(), t_gen.data_ptr(), gs.genes, len(gs.residues), 1, 0,
                               keepalive=(t_res, t_off, t_gen))
    done = PangeneNative.open()                                           # ... and one whose build was finished: preprocessed, and dist
    ptr, records, _ = done.dist_preprocess_begin(K, t_res.data_ptr(), t_off.data_ptr(), t_gen.data_ptr(), gs.genes, len(gs.residues), 1, 0,
                                                 keepalive=(t_res, t_off, t_gen))
    post = torch.empty(max(records, 1) * 2, dtype=torch.int32, device=dev)
    done.copy_device(post.data_ptr(), ptr, records * 8)
    done.dist_preprocess_finish(post.data_ptr(), records, done.run_weights, keepalive=post)
    shard = PangeneNative.open()
    shard.set_genome_shard([0, 2])
    shard.preprocess(K, gs.residues, gs.offsets, gs.genome_of)
    low = PangeneNative.open()
    low.set_option("low_memory", 1)
    low.preprocess(K, gs.residues, gs.offsets, gs.genome_of)
    return dict(zip(COLUMNS + ("single-GPU, finished",), (fresh, cplx, dist, shard, low, done)))


def test_every_yes_cell_of_the_table_is_a_state_refusal(gene_set):
    from pandelos_amd import _lib
    res, off = _new_genes(gene_set)
    ctxs = _contexts(gene_set)
    try:
        for entry, row in TABLE.items():
            for column, needs in zip(COLUMNS, row):
                if not needs:
                    continue
                rc, msg = _call(ctxs[column], entry, res, off, len(off) - 1)
                print(f"{entry} / {column}: rc={rc} {msg!r}")
                assert rc == _lib.PDL_ERR_STATE, (entry, column, rc, msg)
                assert entry in msg, (entry, column, msg)
                if column == "single-GPU":                                # (the begun build is refused as not built: the finished one as multi-GPU)
                    rc, msg = _call(ctxs["single-GPU, finished"], entry, res, off, len(off) - 1)
                    print(f"{entry} / {column}, finished: rc={rc} {msg!r}")
                    assert rc == _lib.PDL_ERR_STATE and entry in msg and "multi-GPU" in msg, (entry, rc, msg)
                if column == "no shard":
                    assert "shard" in msg, (entry, msg)
                if column == "stream held":
                    assert "low_memory" in msg, (entry, msg)
        # the two pointers a caller is given to the edge-list forms
        assert "pdl_families_of_edges" in _call(ctxs["no shard"], "pdl_compute_families", res, off, len(off) - 1)[1]
        assert "pdl_placement_of_edges" in _call(ctxs["no shard"], "pdl_place_query", res, off, len(off) - 1)[1]
    finally:
        for nat in ctxs.values():
            nat.close()


def test_gene_arguments_are_refused_and_the_context_is_left_alone(gene_set):
    from oracle import binding as ob
    from pandelos_amd import _lib
    from pandelos_amd.pangene_native import PangeneNative
    gs = gene_set
    res, off = _new_genes(gs)
    n = len(off) - 1
    falling = off.copy()
    falling[2] = falling[1] - 1                                           # offsets decrease at gene 1
    nat = PangeneNative.from_arrays(K, gs.residues, gs.offsets, gs.genome_of)
    try:
        for entry in GENE_ENTRIES:
            cases = {"NULL offsets": _call(nat, entry, res, None, n), "no gene": _call(nat, entry, res, off, 0),
                     "offsets decrease": _call(nat, entry, res, falling, n), "NULL residues": _call(nat, entry, res, off, n, null_res=True)}
            for what, (rc, msg) in cases.items():
                print(f"{entry} / {what}: rc={rc} {msg!r}")
                assert rc == _lib.PDL_ERR_ARGUMENT, (entry, what, rc, msg)
                assert entry in msg, (entry, what, msg)
            assert "gene 1" in cases["offsets decrease"][1], cases["offsets decrease"][1]
        # the refusals have not disturbed the context
        ora = ob.Oracle(gs.residues, gs.offsets, gs.genome_of, K)
        assert nat.cost.total_cost == ora.total_cost
        for g in range(gs.genomes):
            H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), ora.scores(g), f"genome {g} after the refusals")
    finally:
        nat.close()
