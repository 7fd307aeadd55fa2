"""Who owns K-bbh's buffers on the device (pandelos_amd/csrc/pdl_bbh.hip: the context's BbhBufs and K-place's).

K-bbh runs over three kinds of cells — the context's genome tasks, a query block, a chunk of queries — through one host body and
two sets of buffers.  pdl_compute_families reads the context's own edge lists on the device long after they were written, so
nothing a placement or a caller's K-fam run does in between may touch them.  One context goes through all of it in a row; every
answer is held against the CPU references — the oracle's Scores blocks through the restated filter (tests/bbh_sets.py), the
script's walk of the network (tests/test_place_cpu.py, tests/test_gpu_families.py) — and against fresh contexts that are asked
one thing each."""
import numpy as np
import pytest

from tests import bbh_sets as B
from tests import helpers as H
from tests.test_gpu_families import _assert_same as assert_families, _script_view as families_script_view
from tests.test_gpu_place_batch import assert_same
from tests.test_place_cpu import assert_placement, script_view

pytestmark = pytest.mark.gpu
# tests/bbh_sets.py's "batch": five genomes with chains of paralogs, so that every genome's task — and each of the last two as a
# query of the first three — leaves edges of both phases (a set of pandelos_amd.synth's leaves no phase-2 edge at this size)
NAME = "batch"
BASE, QUERIES = B.BATCH_BASE, B.ALL_BRANCHES["batch"]


def _native(gs, k):
    from pandelos_amd.pangene_native import PangeneNative
    return PangeneNative.from_arrays(k, gs.residues, gs.offsets, gs.genome_of)


def _oracle_edges(gs, k):
    """Per genome of `gs` the edges of its task, from the CPU oracle's block through the restated filter."""
    return [B.edges_of_cells(b, B.filter_cells(b)) for b in B.oracle_blocks(gs, k)]


def _assert_edges(got, want, label):
    for f, x, y in zip(("src", "dst", "score"), got, want):
        assert len(x) == len(y) and np.array_equal(np.asarray(x, np.int64) if f != "score" else H.raw(np.asarray(x, np.float32)),
                                                   np.asarray(y, np.int64) if f != "score" else H.raw(np.asarray(y, np.float32))), f"{label}: {f} differs"


def _edge_bytes(parts):
    return [tuple(H.raw(np.ascontiguousarray(a)).tobytes() for a in p) for p in parts]


@pytest.fixture(scope="module")
def case():
    """The set, its base (three genomes) and the two held-out genomes as queries, with everything the CPU says about them."""
    gs, k = B.gene_set(NAME), B.K
    assert (np.diff(gs.genome_of.astype(np.int64)) >= 0).all()                 # genome-major: a held-out last genome keeps its ids
    base = B.subset(gs, list(BASE))
    N, G = base.genes, len(BASE)
    base_edges = _oracle_edges(base, k)
    bs, bd = (np.concatenate([e[i] for e in base_edges]) for i in (0, 1))
    queries, q_edges, q_placements = [], [], []
    for q in QUERIES:
        union = B.subset(gs, list(BASE) + [q])
        off = union.offsets.astype(np.int64)
        queries.append((union.residues[off[N]:].copy(), (off[N:] - off[N]).astype(np.uint64)))
        e = _oracle_edges(union, k)[G]                                         # the query's task: ids of its own union
        q_edges.append(e)
        q_placements.append(script_view(bs, bd, base.genome_of.tolist(), union.genes - N, e[0], e[1]))
    appended = B.subset(gs, list(BASE) + [QUERIES[0]])
    ae = _oracle_edges(appended, k)
    fam_appended = families_script_view(np.concatenate([e[0] for e in ae]), np.concatenate([e[1] for e in ae]), appended.genome_of.tolist(), appended.genes)
    fam_base = families_script_view(bs, bd, base.genome_of.tolist(), N)
    return dict(k=k, base=base, appended=appended, queries=queries, base_edges=base_edges, q_edges=q_edges, q_placements=q_placements,
                fam_base=fam_base, fam_appended=fam_appended)


def _check_placement(pl, case, j, label):
    want_e, want = case["q_edges"][j], case["q_placements"][j]
    _assert_edges((pl["src"], pl["dst"], pl["score"]), want_e, label + " vs the oracle's edges")
    assert_placement(pl, want, label + " vs the script")


def test_placements_and_a_callers_families_leave_the_contexts_edges_alone(case):
    k, base, queries, G = case["k"], case["base"], case["queries"], len(BASE)
    nat = _native(base, k)
    # 2. the context's own edges and families
    first = [nat.generate_edges_part(g) for g in range(G)]
    for g in range(G):
        _assert_edges(first[g], case["base_edges"][g], f"genome {g}")
    for src, dst, _ in first:                                                  # both kinds, in every task
        intra = base.genome_of[np.asarray(src)] == base.genome_of[np.asarray(dst)]
        assert intra.any() and not intra.all()
    assert_families(nat.generate_families(), case["fam_base"], "the base's families")
    # 3. placements over K-place's own buffers: a batch in one chunk, in two, a single query
    whole = nat.place_batch(queries)
    assert nat.last_place_batch_info["chunks"] == 1
    nat.set_option("query_batch_bytes", 1)
    parts = nat.place_batch(queries)
    assert nat.last_place_batch_info["chunks"] == 2
    single = nat.place_query(*queries[0])
    assert all(pl["edges_phase1"] > 0 and len(pl["src"]) > pl["edges_phase1"] for pl in whole)                      # both kinds again
    # 4. a caller's list overwrites K-fam's work buffers
    assert nat.families_of_edges([0, 1], [1, 2], np.zeros(3, np.uint32))["families"] == 1
    # 5. the context's edges as they were
    second = [nat.generate_edges_part(g) for g in range(G)]
    assert _edge_bytes(second) == _edge_bytes(first)
    # the placements: against the CPU, and against fresh contexts asked one thing each
    for j in range(len(queries)):
        _check_placement(whole[j], case, j, f"one chunk, query {j}")
        _check_placement(parts[j], case, j, f"two chunks, query {j}")
    _check_placement(single, case, 0, "single query")
    fresh = _native(base, k)
    for j, pl in enumerate(fresh.place_batch(queries)):
        assert_same(whole[j], pl, f"one chunk, query {j} vs a fresh context")
    fresh.close()
    fresh = _native(base, k)
    fresh.set_option("query_batch_bytes", 1)
    for j, pl in enumerate(fresh.place_batch(queries)):
        assert_same(parts[j], pl, f"two chunks, query {j} vs a fresh context")
    assert fresh.last_place_batch_info["chunks"] == 2
    fresh.close()
    fresh = _native(base, k)
    assert_same(single, fresh.place_query(*queries[0]), "single query vs a fresh context")
    fresh.close()
    # 6. K-bbh and K-fam anew over the context's own buffers, for the union
    nat.append(*queries[0])
    got = nat.generate_families()
    assert_families(got, case["fam_appended"], "after the append vs the script")
    union = _native(case["appended"], k)
    assert_families(got, union.generate_families(), "after the append vs a context preprocessed on the union")
    for g in range(G + 1):
        assert _edge_bytes([nat.generate_edges_part(g)]) == _edge_bytes([union.generate_edges_part(g)]), f"genome {g} after the append"
    union.close()
    nat.close()
