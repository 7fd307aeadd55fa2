"""Builds, joins and queries of sets with 2^22 genes and more (tests/wide_id_sets.py), where the library leaves its packed forms:
range_plan's 8-byte ranges, the 55-bit key of K-order (pack_ok), the 8-byte put-aside entries (defer_wide), tier 0, the sender
ranges of a multi-GPU build, the query's packed key.  DESIGN.md section 3, "Sets of 2^22 genes and more", lists the switches and
which test here crosses which.  tests/test_wide_id_sets_cpu.py shows on the oracle that the sets reach the cases.

Every comparison is bit for bit against the CPU oracle's values of the case (made once per process); a fresh build on the device is
at most a second witness beside them.  The contexts of "above" and "below" are made once per module: a context of this size
allocates tier 3's tables again, 20 bytes x N x at least 64 workgroups."""
import contextlib

import numpy as np
import pytest

from tests import helpers as H
from tests import wide_id_sets as W

pytestmark = pytest.mark.gpu
B = W.B
DEFAULTS = (("join_tier1", -1), ("join_tier0", -1), ("join_tiny_tier2", 0), ("sift_threshold", 1), ("aside_test_reload", 0))


def _native(c, options=(), shard=None):
    from tests.test_gpu_query import _native as make
    return make(c.k, *c.arrays, options=options, shard=shard)


@pytest.fixture(scope="module")
def above():
    nat = _native(W.case("above"))
    yield nat
    nat.close()


@pytest.fixture(scope="module")
def below():
    nat = _native(W.case("below"))
    yield nat
    nat.close()


@contextlib.contextmanager
def _options(nat, *pairs):
    """the options set, and back at their defaults afterwards (any option marks the scores stale: the next block is a new pass)"""
    try:
        for name, v in pairs:
            nat.set_option(name, v)
        yield nat
    finally:
        for name, v in DEFAULTS:
            nat.set_option(name, v)


def _assert_blocks(get, c, label, genomes=None):
    for g in (range(c.genomes) if genomes is None else genomes):
        H.assert_scores_equal(get(g).as_dict(), c.want[g], f"{label} genome {g}")


def _assert_counters(cost, c, label):
    assert (cost.sequences, cost.genomes) == (c.n, c.genomes), label
    assert (cost.groups, cost.shared_records, cost.dictionary_records) == (*W.shared_groups(c), len(c.dictionary)), label


def _assert_build(nat, c, label):
    """everything pdl_preprocess leaves, and every genome's block"""
    assert nat.cost.total_cost == c.total_cost, label
    _assert_counters(nat.cost, c, label)
    ranks, seqs, counts = nat.dictionary()
    d = c.dictionary
    assert np.array_equal(ranks, d["rank"]) and np.array_equal(seqs, d["seq"]) and np.array_equal(counts, d["count"]), f"{label}: dictionary"
    cost, kl = nat.sequence_costs()
    assert np.array_equal(cost, c.total_visited) and np.array_equal(kl, c.kseq), f"{label}: sequence costs"
    assert [nat.genome_cost(g) for g in range(c.genomes)] == c.genome_cost, label
    nat.score_all()
    _assert_blocks(nat.generate_scores_part, c, label)


# ---- the whole build ----------------------------------------------------------------------------------------------------------------
def test_the_whole_build_below(below):
    _assert_build(below, W.case("below"), "below")
    tm = below.timings()
    assert tm["scored_rows"] == B - 1 and tm["aside_repeats"] == 0 and tm["aside_reloads"] == 0


def test_the_whole_build_at():
    c = W.case("at")
    nat = _native(c)
    _assert_build(nat, c, "at")
    assert nat.timings()["scored_rows"] == B
    with _options(nat, ("join_tier0", 1)):               # the first size at which tier 0 must stay out, even asked for
        _assert_blocks(nat.generate_scores_part, c, "at, tier 0 asked for", genomes=(1, 2))
        tm = nat.timings()
    assert tm["tier1_rows"] == tm["scored_rows"] == B
    nat.close()


def test_the_whole_build_above(above):
    c = W.case("above")
    _assert_build(above, c, "above")
    got = above.generate_scores_part(1).as_dict()
    assert (got["column"] >= B).any() and (got["column"] < B).any() and (got["row"] < B).any() and (got["row"] >= B).any()


# ---- the tiers on "above" -----------------------------------------------------------------------------------------------------------
def test_the_default_tiers_above(above):
    """tier 1 (1024 slots + filter, 16-byte put-aside entries) takes every row; nothing reaches tier 3"""
    c = W.case("above")
    with _options(above, ("join_tier1", -1)):           # (any option: a new pass)
        _assert_blocks(above.generate_scores_part, c, "above, default tiers", genomes=(1, 2))
        tm = above.timings()
    assert tm["tier1_rows"] == tm["scored_rows"] == c.n and tm["overflow_rows"] == 0 and tm["aside_reloads"] == 0 and tm["aside_repeats"] == 0


def test_every_row_through_tier_2_above(above):
    c = W.case("above")
    with _options(above, ("join_tier1", 0)):
        _assert_blocks(above.generate_scores_part, c, "above, tier 2 alone")
        tm = above.timings()
    assert tm["tier1_rows"] == 0 and tm["tier2_rows"] == c.n and tm["overflow_rows"] == 0


def test_wide_rows_overflow_into_tier_3_above(above):
    """the smallest tier-1 table (320 keys) in front of the tiny tier 2 (384 keys): a member of family big meets the members above
    it, gene 25 all 600 of them and the first 200 of genome 1 more than 400 each: tier 3's direct-addressed tables, laid out by N,
    take them"""
    c = W.case("above")
    with _options(above, ("join_tier1", 9), ("join_tiny_tier2", 1)):
        _assert_blocks(above.generate_scores_part, c, "above, tier 1 = 9, tiny tier 2")
        tm = above.timings()
    assert tm["tier1_rows"] == c.n and tm["tier2_rows"] >= tm["overflow_rows"] >= 100, tm
    assert tm["aside_repeats"] == 0


def test_tier_0_stays_out_above(above):
    """forced on, the partition tier still has no packed ranges to read: its keys and its hash take 22-bit ids"""
    c = W.case("above")
    with _options(above, ("join_tier0", 1)):
        _assert_blocks(above.generate_scores_part, c, "above, tier 0 asked for")
        tm = above.timings()
    assert tm["tier1_rows"] == tm["scored_rows"] == c.n                # (with tier 0 in front: the rows it handed on, fewer)


def test_no_pass_is_repeated_above(above):
    """the 16-byte put-aside entries name row and launch in full: the canary never asks for a repeat"""
    c = W.case("above")
    with _options(above, ("aside_test_reload", 1)):
        _assert_blocks(above.generate_scores_part, c, "above, aside_test_reload", genomes=(1, 2))
        tm = above.timings()
    assert tm["aside_repeats"] == 0 and tm["aside_reloads"] == 0


# ---- "below": the last packed size, at the largest 22-bit ids ------------------------------------------------------------------------
def test_one_pass_is_repeated_below(below):
    c = W.case("below")
    with _options(below, ("aside_test_reload", 1)):
        _assert_blocks(below.generate_scores_part, c, "below, aside_test_reload")
        tm = below.timings()
    assert tm["aside_repeats"] == 1 and tm["aside_reloads"] == 0


@pytest.mark.parametrize("sift_threshold", [1, 0])
def test_tier_0_below(below, sift_threshold):
    """tier 0's hash of a column and its inverse at ids up to 2^22 - 2; the rows of family big (57 ranges of 600: more than a cycle's
    8192 lookups) are handed on to the filter tier"""
    c = W.case("below")
    with _options(below, ("join_tier0", 1), ("sift_threshold", sift_threshold)):
        _assert_blocks(below.generate_scores_part, c, f"below, tier 0, sift_threshold {sift_threshold}")
        tm = below.timings()
    assert 0 < tm["tier1_rows"] < tm["scored_rows"] == c.n and tm["aside_reloads"] == 0, tm


# ---- genome shard and batches ---------------------------------------------------------------------------------------------------------
def test_genome_shard_and_reshard_above():
    c = W.case("above")
    nat = _native(c, shard=[1])
    assert nat.cost.total_cost == c.genome_cost[1]
    _assert_counters(nat.cost, c, "above, shard [1]")
    _assert_blocks(nat.generate_scores_part, c, "above, shard [1]", genomes=(1,))
    assert nat.genome_cost(1) == c.genome_cost[1]
    nat.set_genome_shard([0, 2])
    _assert_blocks(nat.generate_scores_part, c, "above, resharded to [0, 2]", genomes=(0, 2))
    assert [nat.genome_cost(g) for g in (0, 2)] == [c.genome_cost[0], c.genome_cost[2]] and nat.timings()["reshard_ms"] > 0
    nat.close()


@pytest.mark.parametrize("low_memory", [0, 1])
def test_genome_batches_of_one_above(low_memory):
    from pandelos_amd.pangene_native import PangeneNative
    c = W.case("above")
    nat = PangeneNative.open()
    costs = []
    for g, s in nat.scores_in_batches(c.k, *c.arrays, 1, low_memory=bool(low_memory)):
        H.assert_scores_equal(s.as_dict(), c.want[g], f"above in batches of one, low_memory {low_memory}, genome {g}")
        costs.append(nat.genome_cost(g))
    assert costs == c.genome_cost
    nat.close()


# ---- ranks together --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sender_ranges", [True, False])
@pytest.mark.parametrize("world", [2, 3])
def test_ranks_together_above(world, sender_ranges):
    """at 2^22 genes the senders' tuples (gene ids of 22 bits) are off: a build that asked for them falls back to the owners"""
    from tests.test_gpu_dist import _local
    c = W.case("above")
    label = f"above W={world}, sender ranges asked for: {sender_ranges}"
    lr, cost = _local(world, *c.arrays, c.k, sender_ranges=sender_ranges)
    assert lr.used_sender_ranges is False, label
    assert lr.total_cost == c.total_cost, label
    assert [lr.genome_cost(g) for g in range(c.genomes)] == c.genome_cost, label
    for n in lr.ranks:
        _assert_counters(n.cost, c, label)
    lr.score_all()
    _assert_blocks(lr.generate_scores_part, c, label)
    lr.close()


# ---- query and query batch -------------------------------------------------------------------------------------------------------------
def _short_query():
    """genes without a k-mer: empty, and of k - 1 residues"""
    lens = np.array([0, W.K - 1, W.K - 1, 0, W.K - 1], np.int64)
    off = np.zeros(len(lens) + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    return np.full(int(off[-1]), W.FILLER_LETTER, np.uint8), off


def test_query_and_query_batch_above():
    """genome 2 as the query of the base of genomes 0 and 1: the union IS the set, so the block is the oracle's of genome 2.  The
    union's column count is past 2^22 (pack_ok = 0 in the query's K-order), and the LDS table is keyed by columns on both sides"""
    from oracle import binding as ob
    from tests.test_gpu_query import _native as make, _union
    c = W.case("above")
    base, query = W.base_and_query(c, 2)
    n_q = len(query[1]) - 1
    assert len(base[2]) >= B and len(base[2]) + n_q == c.n
    nat = make(c.k, *base)
    got = nat.query_scores(*query).as_dict()
    H.assert_scores_equal(got, c.want[2], "above, genome 2 as the query")
    assert nat.last_query_info["genome_cost"] == c.genome_cost[2]
    info = nat.last_query_join_info
    assert info["rows"] == n_q and info["overflow_rows"] == 0 and info["hbm_launches"] == 0, info      # every row in the LDS table
    short = _short_query()
    res, off, gen, G = _union(base, short)
    ora = ob.Oracle(res, off, gen, c.k)
    want_short, cost_short = ora.scores(G), int(ora.genome_cost(G))
    ora.close()
    assert want_short["scoresCount"] == 0
    blocks = [b.as_dict() for b in nat.query_batch([query, short, query])]
    H.assert_scores_equal(blocks[0], c.want[2], "above, query batch, first")
    H.assert_scores_equal(blocks[1], want_short, "above, query batch, the short genes")
    H.assert_scores_equal(blocks[2], c.want[2], "above, query batch, third")
    assert [q["genome_cost"] for q in nat.last_query_batch_info["queries"]] == [c.genome_cost[2], cost_short, c.genome_cost[2]]
    info = nat.last_query_join_info
    assert info["rows"] == 2 * n_q + len(short[1]) - 1 and info["overflow_rows"] == 0, info
    assert nat.cost.sequences == len(base[2]) and nat.cost.genomes == 2
    nat.close()


def test_a_query_row_in_the_hbm_tables_above():
    """the hub query's first row meets 4000 columns, all at or above 2^22: it leaves the LDS table for the HBM tables, laid out by
    the union's column count; alone, and between two small queries of a batch"""
    from tests.test_gpu_query import _native as make
    h = W.hub()
    nat = make(h["k"], *h["base"])
    assert nat.cost.sequences == B + W.HUBS
    for label in ("query", "query again"):
        H.assert_scores_equal(nat.query_scores(*h["query"]).as_dict(), h["want"], f"hub {label}")
        assert nat.last_query_info["genome_cost"] == h["genome_cost"]
        info = nat.last_query_join_info
        assert info["rows"] == 3 and info["overflow_rows"] == 1 and info["hbm_launches"] == 1 and info["hbm_workgroups"] == 1, info
    short = _short_query()
    blocks = [b.as_dict() for b in nat.query_batch([short, h["query"], short])]
    H.assert_scores_equal(blocks[1], h["want"], "hub, the middle one of a batch")
    assert blocks[0]["scoresCount"] == 0 and blocks[2]["scoresCount"] == 0
    assert nat.last_query_batch_info["queries"][1]["genome_cost"] == h["genome_cost"]
    info = nat.last_query_join_info
    assert info["rows"] == 3 + 2 * (len(short[1]) - 1) and info["overflow_rows"] == 1, info
    nat.close()


# ---- append and remove across the limit -----------------------------------------------------------------------------------------------
def _assert_context(nat, c, label):
    assert nat.cost.total_cost == c.total_cost, label
    _assert_counters(nat.cost, c, label)
    ranks, seqs, counts = nat.dictionary()
    d = c.dictionary
    assert np.array_equal(ranks, d["rank"]) and np.array_equal(seqs, d["seq"]) and np.array_equal(counts, d["count"]), f"{label}: dictionary"
    cost, kl = nat.sequence_costs()
    assert np.array_equal(cost, c.total_visited) and np.array_equal(kl, c.kseq), f"{label}: sequence costs"
    assert [nat.genome_cost(g) for g in range(c.genomes)] == c.genome_cost, label
    _assert_blocks(nat.generate_scores_part, c, label)


def test_append_lifts_the_base_over_the_limit_and_remove_brings_it_back():
    """a context that holds the packed form (8-byte ranges, costs on demand) gets N >= 2^22 by an append and must hold the other
    form afterwards, and the packed one again after the removal"""
    base, union = W.case("lift"), W.case("lift+")
    rq, oq, _ = W.lift_query()
    nat = _native(base)
    _assert_context(nat, base, "lift: the base")
    nat.append(rq, oq)
    assert nat.cost.sequences == union.n >= B
    _assert_context(nat, union, "lift: base + genome")
    fresh = _native(union)                               # the second witness: a build of the union
    assert nat.cost.as_dict() == fresh.cost.as_dict() and np.array_equal(nat.scores_counts(), fresh.scores_counts())
    assert all(np.array_equal(x, y) for x, y in zip(nat.rank_table(), fresh.rank_table()))
    fresh.close()
    nat.remove([2])
    assert nat.cost.sequences == base.n < B
    _assert_context(nat, base, "lift: the genome removed again")
    nat.append(rq, oq)
    nat.score_all()
    _assert_blocks(nat.generate_scores_part, union, "lift: appended once more, score_all")
    assert nat.timings()["scored_rows"] == union.n
    nat.close()


def test_a_sharded_base_under_the_limit_refuses_the_append_and_stays():
    """an append needs a context built for all genomes (pdl_append_genomes refuses a genome shard): the shard's context of N < 2^22
    must be as it was after the refusal of a genome that would have lifted it"""
    from pandelos_amd import _lib
    base = W.case("lift")
    rq, oq, _ = W.lift_query()
    nat = _native(base, shard=[1])
    _assert_blocks(nat.generate_scores_part, base, "lift: shard [1]", genomes=(1,))
    with pytest.raises(_lib.PdlError) as e:
        nat.append(rq, oq)
    assert e.value.code == _lib.PDL_ERR_STATE
    assert nat.cost.sequences == base.n
    _assert_blocks(nat.generate_scores_part, base, "lift: shard [1] after the refusal", genomes=(1,))
    nat.close()


# ---- families ----------------------------------------------------------------------------------------------------------------------------
def test_families_above(above):
    """K-bbh's edges equal those of the host's filter on the oracle's blocks; K-fam's labels (23 bits: one more radix digit in its
    sorts) equal the host walk over them, and families whose label is at or above 2^22 are among them"""
    from pandelos_amd.pangenes import bbh_edges
    from pandelos_amd.scores import Scores
    from tests.test_gpu_families import _assert_same, _script_view
    c = W.case("above")
    parts = []
    for g in range(c.genomes):
        w = c.want[g]
        want = bbh_edges(Scores(scoresCount=int(w["scoresCount"]), **{f: np.asarray(w[f]) for f in H.FIELDS}))
        got = above.generate_edges_part(g)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"edges of genome {g}"
        assert H.raw(got[2]).tobytes() == H.raw(want[2]).tobytes(), f"edge scores of genome {g}"
        parts.append(want)
    src, dst = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    want = _script_view(src, dst, c.arrays[2].tolist(), c.n)
    _assert_same(above.generate_families(), want, "above")
    labels = want["component_of"][want["is_node"] == 1]
    assert (labels >= B).any() and (labels < B).any()
    for f in W.HIGH:                                     # a family genome 0 lacks: all its ids, and its label, at or above B
        ids = np.flatnonzero(c.family == f)
        assert len(ids) == 2 and ids.min() >= B and (want["component_of"][ids] == ids.min()).all()
