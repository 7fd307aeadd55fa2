"""The group-head bit stays in bit 31 of a posting's count: the write passes of the range stage only read the postings, and every
reader of a count masks the bit (the joins; pdl_get_dictionary and the query kernels always did).

Where an unmasked bit would show.  In the upper-range build (single GPU, the multi-GPU flows) a row walks only the genes ABOVE
it, so a group's head record is never gathered as a posting — but a range whose own count is packed as 1023 reads the true count
from the record in front of it, and for the group's second gene that record is the head.  In genome batches (whole groups for the
genes of a shard) the head is gathered like every other member.  So the sets here plant one k-mer, WWW, in family 0: gene 0 — the
smallest id of the set, the head of that group — holds it `repeat` times, the family's genes in the other genomes once.
A count read with its bit would be 2^31 too large: the scores, percs and tr_percs of family 0's cells would change.

Sets of 4 genomes x 12 genes at k = 3, built the way tests/range_stage_sets.py builds its own; every case against the CPU oracle,
field for field."""
import functools

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

K = 3
GENOMES, FAMS = 4, 12
BODY_LETTERS = np.array([c for c in H.LETTERS if c != ord("W")], dtype=np.uint8)       # Y stays: WWW is not the largest rank


def _head_set(repeat, seed=11, sub=0.08):
    rng = np.random.default_rng(seed)
    bases = [BODY_LETTERS[rng.integers(0, len(BODY_LETTERS), int(rng.integers(30, 101)))] for _ in range(FAMS)]
    genes, gen, fam = [], [], []
    for g in range(GENOMES):
        for f, base in enumerate(bases):
            s = base.copy()
            m = rng.random(len(s)) < sub
            s[m] = BODY_LETTERS[rng.integers(0, len(BODY_LETTERS), int(m.sum()))]
            if f == 0:                                   # the planted k-mer: `repeat` times in gene 0, once in its family elsewhere
                s = np.concatenate([s[:len(s) // 2], H.stretch([ord("W")], repeat if g == 0 else 1, K), s[len(s) // 2:]])
            genes.append(s); gen.append(g); fam.append(f)
    return H._as_gene_set(genes, gen, fam)


@functools.lru_cache(maxsize=None)
def _case(repeat) -> H.OracleCase:
    """The set and the oracle's answer; made once, never changed.  Checked for what it is built for."""
    c = H.OracleCase(_head_set(repeat), K)
    r, gid, start, size = H.rank_groups(c.dictionary)
    planted = [i for i in range(len(start)) if r["seq"][start[i]] == 0 and r["count"][start[i]] == repeat]
    assert len(planted) == 1                             # one group whose head is gene 0 with the planted count ...
    i = planted[0]
    assert size[i] == GENOMES and r["seq"][start[i]:start[i] + size[i]].tolist() == [g * FAMS for g in range(GENOMES)]
    assert r["count"][start[i] + 1:start[i] + size[i]].tolist() == [1] * (GENOMES - 1)
    assert start[i] + size[i] < len(r)                   # ... and it is not the dictionary's last group (no fold involved)
    return c


def _assert_blocks(get, c, label):
    for g in range(c.genomes):
        H.assert_scores_equal(get(g).as_dict(), c.want[g], f"{label} genome {g}")


# ---- (a) the head has a count of 2 or more ---------------------------------------------------------------------------------------
REPEAT_A = 3


def test_head_with_a_count_above_one_whole_build():
    from tests.test_gpu_query import _native
    c = _case(REPEAT_A)
    nat = _native(c.k, *c.arrays)
    assert nat.cost.total_cost == c.total_cost
    _assert_blocks(nat.generate_scores_part, c, "whole build")
    nat.close()


@pytest.mark.parametrize("repeat", [REPEAT_A, 1100])
def test_head_with_a_count_above_one_genome_batches_of_one(repeat):
    """whole groups for the genes of the batch: the head record is gathered as a posting, by every row of the other batches"""
    from pandelos_amd.pangene_native import PangeneNative
    c = _case(repeat)
    nat = PangeneNative.open()
    costs = []
    for g, s in nat.scores_in_batches(c.k, *c.arrays, 1, low_memory=False):
        H.assert_scores_equal(s.as_dict(), c.want[g], f"repeat {repeat}, batches of one, genome {g}")
        costs.append(nat.genome_cost(g))
    assert costs == c.genome_cost
    nat.close()


@pytest.mark.parametrize("ranges", ["sender", "owner"])
def test_head_with_a_count_above_one_two_ranks(ranges):
    from tests.test_gpu_dist import _local
    c = _case(REPEAT_A)
    lr, cost = _local(2, *c.arrays, c.k, sender_ranges=ranges == "sender")
    assert lr.used_sender_ranges == (ranges == "sender")
    assert lr.total_cost == c.total_cost
    assert [lr.genome_cost(g) for g in range(c.genomes)] == c.genome_cost
    lr.score_all()
    _assert_blocks(lr.generate_scores_part, c, f"W=2 {ranges} ranges")
    lr.close()


# ---- (b) the head's count is read from the posting: 1023 repeats and more --------------------------------------------------------
@pytest.mark.parametrize("repeat", [1023, 1100])
@pytest.mark.parametrize("options", [[("join_tier0", 1)], [("join_tier0", 1), ("sift_threshold", 0)]] +
                                    [[("join_tier1", t)] for t in (-1, 0, 9, 10, 11, 20, 21)], ids=lambda o: "-".join(f"{n}{v}" for n, v in o))
def test_saturated_count_behind_a_head_through_every_first_tier(repeat, options):
    from tests.test_gpu_query import _native
    c = _case(repeat)
    nat = _native(c.k, *c.arrays, options=options)
    assert nat.cost.total_cost == c.total_cost
    _assert_blocks(nat.generate_scores_part, c, f"repeat {repeat} {options}")
    tm = nat.timings()
    if options[0] == ("join_tier0", 1):
        assert tm["scored_rows"] - tm["tier1_rows"] > 0  # rows stayed in the partition tier
    nat.close()


@pytest.mark.parametrize("ranges", ["sender", "owner"])
def test_saturated_count_behind_a_head_two_ranks(ranges):
    """the range points into the gathered dictionary, whose records carry the bits they travelled with"""
    from tests.test_gpu_dist import _local
    c = _case(1100)
    lr, cost = _local(2, *c.arrays, c.k, sender_ranges=ranges == "sender")
    assert lr.used_sender_ranges == (ranges == "sender") and lr.total_cost == c.total_cost
    lr.score_all()
    _assert_blocks(lr.generate_scores_part, c, f"repeat 1100 W=2 {ranges} ranges")
    lr.close()


# ---- (c) two batches in a row, then the costs and the dictionary -----------------------------------------------------------------
@pytest.mark.parametrize("repeat", [REPEAT_A, 1100])
def test_two_batches_then_costs_and_dictionary(repeat):
    from pandelos_amd.pangene_native import PangeneNative
    c = _case(repeat)
    nat = PangeneNative.open()
    nat.set_genome_shard([0, 1])
    nat.preprocess(c.k, *c.arrays)
    for g in (0, 1):
        H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), c.want[g], f"first batch, genome {g}")
    nat.set_genome_shard([2, 3])                         # the range lists again, from postings the first write pass has read
    for g in (2, 3):
        H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), c.want[g], f"second batch, genome {g}")
        assert nat.genome_cost(g) == c.genome_cost[g]
    cost, kl = nat.sequence_costs()
    mine = np.flatnonzero(c.gs.genome_of >= 2)           # a shard's context keeps the costs of its own genes
    assert np.array_equal(cost[mine], c.total_visited[mine]) and np.array_equal(kl, c.kseq)
    ranks, seqs, counts = nat.dictionary()
    d = c.dictionary
    assert np.array_equal(ranks, d["rank"]) and np.array_equal(seqs, d["seq"]) and np.array_equal(counts, d["count"])      # clean counts
    assert int(counts.max()) == max(repeat, int(d["count"].max()))
    nat.set_genome_shard([0])                            # ... and a third batch after both reads
    H.assert_scores_equal(nat.generate_scores_part(0).as_dict(), c.want[0], "third batch, genome 0")
    nat.close()


def test_whole_build_then_costs_and_dictionary():
    """packed ranges: the per-gene costs are made on demand from the copy of the head bits the write pass filed"""
    from tests.test_gpu_query import _native
    c = _case(1100)
    nat = _native(c.k, *c.arrays)
    cost, kl = nat.sequence_costs()
    assert np.array_equal(cost, c.total_visited) and np.array_equal(kl, c.kseq)
    assert [nat.genome_cost(g) for g in range(c.genomes)] == c.genome_cost
    ranks, seqs, counts = nat.dictionary()
    d = c.dictionary
    assert np.array_equal(ranks, d["rank"]) and np.array_equal(seqs, d["seq"]) and np.array_equal(counts, d["count"])
    _assert_blocks(nat.generate_scores_part, c, "after the cost pass")
    nat.close()


# ---- (d) append one genome, score, remove it, score ------------------------------------------------------------------------------
@pytest.mark.parametrize("repeat", [REPEAT_A, 1100])
def test_append_score_remove_score(repeat):
    from tests.test_gpu_append import _append_vs_union, _assert_oracle
    from tests.test_gpu_query import _split
    from tests.test_gpu_remove import _remaining
    c = _case(repeat)
    res, off, gen = c.arrays
    base, query = _split(res, off, gen, c.genomes - 1)
    nat = _append_vs_union(base, query, c.k, f"repeat {repeat}: append")         # = a build of the union = the oracle (blocks, costs)
    _assert_blocks(nat.generate_scores_part, c, f"repeat {repeat}: appended")   # (the union is the set itself: its last genome came last)
    nat.remove([c.genomes - 1])
    _assert_oracle(nat, *_remaining(res, off, gen, [c.genomes - 1]), c.k, f"repeat {repeat}: removed again")
    nat.close()
