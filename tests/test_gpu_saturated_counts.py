"""K-mers that occur 1023 times or more inside one gene, through every join tier.

The single-GPU build stores a row's ranges packed in 8 bytes, the row's own count of the k-mer in ten bits (gt_pack_range in
pdl_groups.h: min(count, 1023)).  At 1023 the reader takes the true count from the record in front of the range, post[first - 1].y:
    k_join_lds   "unpack"                 every tier-1 table and tier 2
    k_join_hbm   packed and WIDE          tier 3
    k_join_part  the heavy-lookup list    tier 0, fed by both sift forms
    the multi-GPU flows                   the range points into the gathered dictionary (pos_base)
In the upper-range build the first record of a rank-group is nobody's posting: that word, which carried the head bit until the
write pass took it out (gt_take_head), has no other reader.  A bit left behind, a re-read of the wrong posting or a reader that
takes 1023 for the value would change scores, percs and tr_percs of every cell of such a gene and nothing else.

Every case: each genome's block against the CPU oracle, bit for bit and in emission order, and the total cost.  The sets are
checked for what they are built for in tests/test_saturated_sets_cpu.py."""
import functools

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

FAMS = 20
SETS = [(3, 1), (3, 2), (4, 1), (4, 2)]                  # (k, period of the planted stretch)


def _open(case, options=(), flags=0, shard=None):
    from tests.test_gpu_query import _native
    nat = _native(case.k, *case.arrays, flags=flags, options=options, shard=shard)
    return nat


def _score(case, options=(), flags=0, label=""):
    """Build, compare every genome with the oracle -> the timings"""
    nat = _open(case, options, flags)
    assert nat.cost.total_cost == case.total_cost, label
    for g in range(case.genomes):
        H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), case.want[g], f"{label} genome {g}")
    tm = nat.timings()
    nat.close()
    return tm


def _with_gene(gs, gene):
    """`gs` with one more gene at the end of its last genome"""
    from pandelos_amd.synth import GeneSet
    gene = np.asarray(gene, np.uint8)
    return GeneSet(np.concatenate([gs.residues, gene]), np.r_[gs.offsets, gs.offsets[-1] + np.uint64(len(gene))].astype(np.uint64),
                   np.r_[gs.genome_of, gs.genome_of[-1]].astype(np.uint32), np.r_[gs.family_of, -1])


@functools.lru_cache(maxsize=None)
def _case(name):
    """The sets of this file beyond helpers.saturated_case, each with the oracle's answer; made once, never changed."""
    kind, _, arg = name.partition(":")
    if kind in ("sat", "dense"):
        return H.saturated_case(name)
    k, period = (int(x) for x in arg.split(":")[:2])
    gs = H.saturated_case(f"sat:{k}:{period}").gs
    if kind == "sat+short":                              # one gene of 5k k-mers: the set's sift threshold falls below PT_SIFT_T_MIN
        return H.OracleCase(_with_gene(gs, gs.residues[:5 * k + k - 1]), k)
    if kind == "sat+giant":                              # one gene of 2^20 + 5000 residues: 32-bit counters for every row
        rng = np.random.default_rng(12)
        return H.OracleCase(_with_gene(gs, H.LETTERS[rng.integers(0, 20, (1 << 20) + 5000)]), k)
    raise KeyError(name)


# ---- (a) the default plan and every tier-1 table -------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", [-1, 0, 9, 10, 11, 20, 21])
@pytest.mark.parametrize("k,period", SETS)
def test_every_first_tier_reads_the_count_behind_a_saturated_field(k, period, tier):
    case = _case(f"sat:{k}:{period}")
    tm = _score(case, [("join_tier1", tier)], label=f"k {k} period {period} tier {tier}")
    assert tm["aside_reloads"] == 0 and tm["aside_repeats"] == 0
    if tier == 0:
        assert tm["tier2_rows"] == tm["scored_rows"] and tm["overflow_rows"] == 0         # k_join_lds<13, 1024> took every row
    else:
        assert tm["overflow_rows"] == 0                                                   # no row was left for the HBM kernel


def test_canonical_order_with_saturated_counts():
    from pandelos_amd import _lib
    case = _case("sat:3:2")
    nat = _open(case, flags=_lib.PDL_FLAG_CANONICAL_ORDER)
    assert nat.cost.total_cost == case.total_cost
    for g in range(case.genomes):
        got, w = nat.generate_scores_part(g).as_dict(), case.want[g]
        order = np.lexsort((w["column"], w["row"]))
        for f in ("scores", "percs", "tr_percs", "row", "column"):
            assert np.array_equal(H.raw(got[f]), H.raw(np.asarray(w[f])[order])), f"canonical genome {g} {f}"
        for f in ("max_genome_score", "max_genome_score_col", "scoresMaxMappings"):
            assert np.array_equal(H.raw(got[f]), H.raw(w[f])), f"canonical genome {g} {f}"
    nat.close()


def test_a_repeated_pass_reads_the_same_counts():
    """A staging area of 16 cells: the first attempt overflows and the pass is repeated with the size it asked for."""
    _score(_case("sat:4:2"), [("staging_cap", 16)], label="tiny staging")


@pytest.mark.parametrize("tier", [10, 11])
def test_a_pass_repeated_with_wide_put_aside_entries_reads_the_same_counts(tier):
    tm = _score(_case("sat:3:1"), [("join_tier1", tier), ("aside_test_reload", 1)], label=f"tier {tier}, repeated with wide entries")
    assert tm["aside_repeats"] == 1 and tm["aside_reloads"] == 0


# ---- (b) tier 0 forced, both sift forms ----------------------------------------------------------------------------------------
def _sift_t(case):
    """the partition tier's threshold for the whole set (score_plan in pdl_join.hip: min_numerator of the shortest gene)"""
    from tests.test_gpu_sift_threshold import _min_numerator
    return max(2, min(255, _min_numerator(int(case.kseq.min()), case.k)))


@pytest.mark.parametrize("form", ["counters", "bitmaps", "counters_at_2"])
@pytest.mark.parametrize("k,period", SETS)
def test_the_partition_tier_reads_the_count_behind_a_saturated_field(k, period, form):
    from tests.test_gpu_sift_threshold import SIFT_T_MIN
    case = _case(f"sat+short:{k}:{period}" if form == "bitmaps" else f"sat:{k}:{period}")
    assert (_sift_t(case) >= SIFT_T_MIN) == (form != "bitmaps") and case.kseq.min() > 2 * k
    tm = _score(case, [("join_tier0", 1), ("sift_threshold", 0 if form == "counters_at_2" else 1)], label=f"tier 0 {form} k {k} period {period}")
    print(f"tier 0 {form} k {k} period {period}: rows {tm['scored_rows']}, to the filter tier {tm['tier1_rows']}, tier 2 {tm['tier2_rows']}, tier 3 {tm['overflow_rows']}")
    # the last gene of a family has no range of its own: more rows than that stayed in tier 0, some of them with a saturated range
    assert tm["scored_rows"] - tm["tier1_rows"] > FAMS
    assert tm["aside_reloads"] == 0


# ---- (c) tier 3, packed counters -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier1", [0, -1])
def test_the_hbm_kernel_reads_the_count_behind_a_saturated_field(tier1):
    """"join_tiny_tier2": a table of 384 keys in place of tier 2.  Without a first tier ("join_tier1" 0) every row comes to it, and
    the rows of more than 384 columns go on to k_join_hbm: gene i meets the 599 - i genes above it.  Behind the default first tier
    only the rows that tier hands on get that far (its filter keeps the columns sighted once out of its table): same cells."""
    case = _case("dense")
    tm = _score(case, [("join_tier1", tier1), ("join_tiny_tier2", 1)], label=f"dense group, tiny tier 2, tier 1 {tier1}")
    print(f"dense, tier 1 {tier1}: rows {tm['scored_rows']}, tier 2 {tm['tier2_rows']}, tier 3 {tm['overflow_rows']}")
    assert tm["overflow_rows"] >= (case.gs.genes - 385 if tier1 == 0 else 1)


# ---- (d) tier 3, wide counters -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("period", [1, 2])
def test_the_hbm_kernel_with_wide_counters_reads_the_count_behind_a_saturated_field(period):
    case = _case(f"sat+giant:4:{period}")
    tm = _score(case, label=f"wide counters, period {period}")
    assert tm["overflow_rows"] == case.gs.genes


# ---- (e) the 21-bit fields at their bound --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmers,wide", [((1 << 20) - 1, False), (1 << 20, True)])
def test_twins_of_the_longest_gene_the_packed_counters_take(kmers, wide):
    from pandelos_amd.synth import GeneSet
    k = 4
    rng = np.random.default_rng(5)
    giant = H.LETTERS[rng.integers(0, 20, kmers + k - 1)]
    genes = [giant, giant.copy()] + [giant[i * 9973:i * 9973 + 400].copy() for i in range(6)]
    off = np.zeros(len(genes) + 1, np.uint64)
    np.cumsum([len(x) for x in genes], out=off[1:])
    case = H.OracleCase(GeneSet(np.concatenate(genes), off, np.asarray([0, 1, 0, 1, 2, 2, 0, 1], np.uint32), np.zeros(8, np.int64)), k)
    assert case.kseq.max() == kmers
    nat = _open(case)
    assert nat.cost.total_cost == case.total_cost
    got = [nat.generate_scores_part(g).as_dict() for g in range(case.genomes)]
    tm = nat.timings()
    nat.close()
    for g in range(case.genomes):
        H.assert_scores_equal(got[g], case.want[g], f"{kmers} k-mers genome {g}")
    twin = np.flatnonzero((got[0]["row"] == 0) & (got[0]["column"] == 1))
    assert len(twin) == 1
    one = np.float32(1.0).view(np.uint32)
    assert all(H.raw(got[0][f])[twin[0]] == one for f in ("scores", "percs", "tr_percs"))
    if wide:
        assert tm["overflow_rows"] == len(genes)
    else:
        assert tm["overflow_rows"] < tm["scored_rows"]


# ---- (f) the other observables -------------------------------------------------------------------------------------------------
def test_dictionary_and_costs_of_a_saturated_set():
    case = _case("sat:3:1")
    nat = _open(case)
    ranks, seqs, counts = nat.dictionary()
    d = case.dictionary
    assert np.array_equal(ranks, d["rank"]) and np.array_equal(seqs, d["seq"]) and np.array_equal(counts, d["count"])
    assert (counts == 3000).sum() >= FAMS // 4
    cost, kl = nat.sequence_costs()                      # packed ranges: the lazy cost pass (pdl_ensure_costs)
    assert np.array_equal(cost, case.total_visited) and np.array_equal(kl, case.kseq)
    assert [nat.genome_cost(g) for g in range(case.genomes)] == case.genome_cost
    for g in range(case.genomes):                        # ... and scoring after it
        H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), case.want[g], f"after the cost pass, genome {g}")
    ranks, seqs, counts = nat.dictionary()               # the write pass took the head bits out: the counts are still the counts
    assert np.array_equal(counts, d["count"])
    nat.close()


# ---- (g) the fold of the last record meets a saturated count -------------------------------------------------------------------
@pytest.mark.parametrize("tier0", [0, 1])
@pytest.mark.parametrize("variant", ["head", "middle", "same_gene_twice"])
def test_a_folded_last_record_with_a_saturated_count(variant, tier0):
    gs, x = H.fold_saturated_set(variant)
    case = H.OracleCase(gs, 3)
    nat = _open(case, [("join_tier0", tier0)])
    assert nat.cost.total_cost == case.total_cost
    ranks, seqs, counts = nat.dictionary()
    d = case.dictionary
    assert np.array_equal(ranks, d["rank"]) and np.array_equal(seqs, d["seq"]) and np.array_equal(counts, d["count"])
    assert counts[ranks == ranks.max()].tolist() == [3000]
    for g in range(case.genomes):
        H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), case.want[g], f"fold {variant} genome {g}")
    cost, kl = nat.sequence_costs()
    assert np.array_equal(cost, case.total_visited)
    nat.close()


# ---- (h) the flows that do not depend on the packing ---------------------------------------------------------------------------
def test_a_shard_set_before_the_build_matches_the_oracle():
    """16-byte tuples {first posting, postings, own count, group size}: no packed field"""
    case = _case("sat:3:2")
    for shard in ([0, 2], [1, 3]):
        nat = _open(case, shard=shard)
        for g in shard:
            H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), case.want[g], f"shard {shard} genome {g}")
            assert nat.genome_cost(g) == case.genome_cost[g]
        nat.close()


@pytest.mark.parametrize("low_memory", [True, False])
def test_genome_batches_of_one_match_the_oracle(low_memory):
    """every batch puts the head bits back and builds its range lists again"""
    from pandelos_amd.pangene_native import PangeneNative
    case = _case("sat:4:2")
    nat = PangeneNative.open()
    seen = 0
    for g, s in nat.scores_in_batches(case.k, *case.arrays, 1, low_memory=low_memory):
        H.assert_scores_equal(s.as_dict(), case.want[g], f"batches of one, genome {g}")
        seen += 1
    assert seen == case.genomes
    nat.close()


# ---- (i) multi-GPU -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sender_ranges", [True, False])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("k,period", [(3, 1), (4, 2)])
def test_ranks_together_read_the_count_behind_a_saturated_field(k, period, world, sender_ranges):
    from tests.test_gpu_dist import _local
    case = _case(f"sat:{k}:{period}")
    lr, cost = _local(world, *case.arrays, k, sender_ranges=sender_ranges)
    assert lr.used_sender_ranges == sender_ranges        # the ranges come from the rank that holds the run / from the gene's owner
    assert lr.total_cost == case.total_cost
    assert [lr.genome_cost(g) for g in range(case.genomes)] == case.genome_cost
    lr.score_all()
    for g in range(case.genomes):
        H.assert_scores_equal(lr.generate_scores_part(g).as_dict(), case.want[g], f"W={world} sender ranges {sender_ranges} genome {g}")
    lr.close()


# ---- (j) the incremental entry points ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,period", [(3, 2), (4, 1)])
def test_append_then_remove_with_saturated_counts(k, period):
    from tests.test_gpu_append import _append_vs_union, _assert_oracle, _assert_same_context
    from tests.test_gpu_query import _native, _split
    from tests.test_gpu_remove import _remaining
    case = _case(f"sat:{k}:{period}")
    res, off, gen = case.arrays
    base, query = _split(res, off, gen, case.genomes - 1)
    nat = _append_vs_union(base, query, k, f"append k {k} period {period}")      # = a build of the union (blocks, edges, costs) = the oracle
    nat.remove([0])
    rest = _remaining(res, off, gen, [0])
    reb = _native(k, *rest)
    _assert_same_context(nat, reb, f"then remove genome 0, k {k} period {period}")
    _assert_oracle(nat, *rest, k, "after the removal")
    reb.close(); nat.close()


@pytest.mark.parametrize("k,period", [(3, 2), (4, 1)])
def test_query_and_query_batch_with_saturated_counts(k, period):
    from tests.test_gpu_query import _check_against_oracle, _native, _split, _union
    case = _case(f"sat:{k}:{period}")
    res, off, gen = case.arrays
    base, (rq, oq) = _split(res, off, gen, case.genomes - 1)
    # the query must not hold the union's largest-rank k-mer (the fold is not attempted, pandelos_amd.h): genes that do stay out of it
    n_base, o64 = len(base[2]), oq.astype(np.int64)
    genes = [rq[o64[i]:o64[i + 1]] for i in range(len(oq) - 1)]
    while True:
        qoff = np.zeros(len(genes) + 1, np.uint64)
        np.cumsum([len(x) for x in genes], out=qoff[1:])
        query = (np.concatenate(genes).astype(np.uint8), qoff)
        ures, uoff, ugen, G = _union(base, query)
        holders = [h - n_base for h in H.genes_holding_the_largest_kmer(ures, uoff, k) if h >= n_base]
        if not holders:
            break
        genes = [x for i, x in enumerate(genes) if i not in holders]
    assert len(genes) >= FAMS - 4 and G == case.genomes - 1
    nat = _native(k, *base)
    got, ora = _check_against_oracle(nat, base, query, k, f"query k {k} period {period}")
    assert len(got["row"]) > 0
    half = len(genes) // 2
    first = (query[0][:int(qoff[half])], qoff[:half + 1])
    blocks = nat.query_batch([query, first, query])
    H.assert_scores_equal(blocks[0].as_dict(), got, "batch, query 0")
    H.assert_scores_equal(blocks[2].as_dict(), got, "batch, query 2")
    _check_against_oracle(nat, base, first, k, "the first half alone")
    H.assert_scores_equal(blocks[1].as_dict(), nat.query_scores(*first).as_dict(), "batch, query 1")
    nat.close()
