"""K-bbh (pandelos_amd/csrc/pdl_bbh.hip) behind each of its three locators, on the sets of tests/bbh_sets.py, which reach every
branch of the filter (tests/test_bbh_branches_cpu.py holds them to that).

The reference everywhere is pangenes.bbh_edges applied to the CPU ORACLE's Scores block of the set in question — never to the
device's own block: src, dst and the raw bits of score, in order.
  * BbhTasks: whole contexts, scoring options, genome shards set before the build and changed on a built dictionary (task indices
    that differ from genome ids), the native host with and without --genome-batch, append, remove;
  * BbhQueryBlock: place_query with the all-branches genome held out;
  * BbhQueryChunk: place_batch with both all-branches genomes held out, in one chunk and in a chunk each."""
import subprocess

import numpy as np
import pytest

from pandelos_amd import pangenes as PH
from pandelos_amd.scores import Scores
from tests import bbh_sets as B
from tests import helpers as H
from tests.test_gpu_query import _native

pytestmark = pytest.mark.gpu
_REF = {}


def reference(name, genomes=None):
    """bbh_edges of every oracle block of set `name` (or of its subset of `genomes`); made once, never changed."""
    key = (name, None if genomes is None else tuple(genomes))
    if key not in _REF:
        _REF[key] = [PH.bbh_edges(Scores(**{f: blk[f] for f in ("scoresCount",) + H.FIELDS})) for blk in B.blocks(name, genomes)]
    return _REF[key]


def assert_edges(got, want, label):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"{label}: the edges' genes differ from the reference's"
    assert np.asarray(got[2]).dtype == np.float32 and H.raw(got[2]).tobytes() == H.raw(want[2]).tobytes(), f"{label}: an edge's score bits differ"


def assert_context(nat, want, genomes, label):
    assert len(want) == nat.cost.genomes, label
    for g in genomes:
        assert_edges(nat.generate_edges_part(g), want[g], f"{label}, genome {g}")


def open_set(gs, options=(), shard=None):
    return _native(B.K, gs.residues, gs.offsets, gs.genome_of, options=options, shard=shard)


def reference_net(name):
    from oracle import pangenes_host as oh
    gs, blks = B.gene_set(name), B.blocks(name)
    return "".join(oh.build_net(lambda g: blks[g], gs.genomes, gs.genes))


def query_of(gs, genome):
    q = B.subset(gs, [genome])
    return q.residues, q.offsets


# ---- BbhTasks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(B.SETS))
def test_whole_context(name):
    gs = B.gene_set(name)
    nat = open_set(gs)
    assert_context(nat, reference(name), range(gs.genomes), name)
    assert "".join(PH.run(nat, gs.genomes)) == reference_net(name), f"{name}: the .net text"
    nat.close()


@pytest.mark.parametrize("option,value", [("host_mirror", 0), ("staging_cap", 16), ("aside_test_reload", 1), ("join_tier0", 0), ("join_tier0", 1)])
def test_scoring_options_change_no_edge(option, value):
    name = "batch"
    gs = B.gene_set(name)
    # (the put-aside lists that the reload switch is about exist in the filter tiers 9-11 only)
    nat = open_set(gs, options=([("join_tier1", 10)] if option == "aside_test_reload" else []) + [(option, value)])
    assert_context(nat, reference(name), range(gs.genomes), f"{name}, {option} = {value}")
    tm = nat.timings()
    if option == "staging_cap":                       # far below the cells of one row: the pass ran twice
        plain = open_set(gs)
        plain.generate_edges_part(0)
        assert tm["join_launches"] > plain.timings()["join_launches"]
        plain.close()
    if option == "aside_test_reload":
        assert tm["aside_repeats"] == 1
    nat.close()


@pytest.mark.parametrize("shard", [[1, 3], [0, 2, 4]])
def test_shard_set_before_the_build(shard):
    """A shard that does not start at genome 0 and its complement: task indices are not genome ids, and inter_max's rows are the
    shard's."""
    from pandelos_amd import _lib
    name = "batch"
    gs = B.gene_set(name)
    nat = open_set(gs, shard=shard)
    assert_context(nat, reference(name), shard, f"{name}, shard {shard}")
    with pytest.raises(_lib.PdlError):
        nat.generate_edges_part(next(g for g in range(gs.genomes) if g not in shard))
    nat.close()


def test_shards_changed_on_a_built_dictionary():
    name = "batch"
    gs = B.gene_set(name)
    nat = open_set(gs, shard=[1, 3])
    for shard in ([1, 3], [0, 2], [4], [3], list(range(gs.genomes)), [2, 4]):
        nat.set_genome_shard(shard)
        assert_context(nat, reference(name), shard, f"{name}, shard {shard} on a dictionary built for [1, 3]")
    nat.close()


@pytest.mark.parametrize("per_batch", [0, 1, 3])
def test_native_host_in_genome_batches(per_batch, tmp_path):
    from pandelos_amd import _lib
    name = "chains"
    gs = B.gene_set(name)
    faa, net = tmp_path / "in.faa", tmp_path / "out.net"
    gs.write_faa(faa)
    cmd = [str(_lib.LIB_DIR / "pangenes"), "-i", str(faa), "-k", str(B.K), "-o", str(net)] + (["--genome-batch", str(per_batch)] if per_batch else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert ("genome batches of" in p.stdout) == bool(per_batch)
    assert net.read_text() == reference_net(name)


def test_append_of_the_all_branches_genome():
    """The base without the genome that reaches every branch, then that genome appended: every genome's edges are the oracle's for
    the union, and so are the families K-fam makes of them."""
    from tests.test_gpu_families import _assert_same, _script_view
    name, held = "single", B.ALL_BRANCHES["single"][0]
    gs = B.gene_set(name)
    nat = open_set(B.subset(gs, [g for g in range(gs.genomes) if g != held]))
    nat.append(*query_of(gs, held))
    assert nat.cost.genomes == gs.genomes and nat.cost.sequences == gs.genes
    want = reference(name)
    assert_context(nat, want, range(gs.genomes), f"{name}, genome {held} appended")
    src, dst = (np.concatenate([w[i] for w in want]) for i in (0, 1))
    _assert_same(nat.generate_families(), _script_view(src, dst, gs.genome_of.tolist(), gs.genes), f"{name}, genome {held} appended: families")
    nat.close()


def test_removal_of_a_middle_genome():
    name, gone = "batch", 2
    gs = B.gene_set(name)
    rest = [g for g in range(gs.genomes) if g != gone]
    nat = open_set(gs)
    nat.remove([gone])
    assert nat.cost.genomes == len(rest) and nat.cost.sequences == B.subset(gs, rest).genes
    assert_context(nat, reference(name, rest), range(len(rest)), f"{name}, genome {gone} removed")
    nat.close()


# ---- BbhQueryBlock, BbhQueryChunk -------------------------------------------------------------------------------------------
def test_place_query_of_the_all_branches_genome():
    name, held = "single", B.ALL_BRANCHES["single"][0]
    gs = B.gene_set(name)
    nat = open_set(B.subset(gs, [g for g in range(gs.genomes) if g != held]))
    pl = nat.place_query(*query_of(gs, held))
    assert_edges((pl["src"], pl["dst"], pl["score"]), reference(name)[held], f"{name}, genome {held} as a query")
    nat.close()


@pytest.mark.parametrize("budget,chunks", [(None, 1), (1, 2)])
def test_place_batch_of_both_all_branches_genomes(budget, chunks):
    """Each query against the oracle of its own union with the base; with a budget of one byte, a chunk each."""
    name = "batch"
    gs = B.gene_set(name)
    nat = open_set(B.subset(gs, list(B.BATCH_BASE)))
    if budget is not None:
        nat.set_option("query_batch_bytes", budget)
    pls = nat.place_batch([query_of(gs, q) for q in B.ALL_BRANCHES[name]])
    assert nat.last_place_batch_info["chunks"] == chunks
    for q, pl in zip(B.ALL_BRANCHES[name], pls):
        want = reference(name, B.BATCH_BASE + (q,))[len(B.BATCH_BASE)]
        assert_edges((pl["src"], pl["dst"], pl["score"]), want, f"{name}, genome {q} as a query of a batch in {chunks} chunk(s)")
    nat.close()
