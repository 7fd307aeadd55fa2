"""The host side of the range stage (pdl_dict.hip: K-groups + K-ranges + K-cost) at its corner cases, through each of its entry
paths: a shard that builds no range at all (buffers for max(count, 1)), a run that makes no tuple, an empty inbox, a rank that owns
no genome.  The sets are tests/range_stage_sets.py; tests/test_range_stage_sets_cpu.py shows on the oracle that they reach the cases.

Every path: each genome's Scores block, the per-genome costs, the total cost, the groups and the shared records equal the CPU
oracle's, bit for bit.  (Tuples of 16 bytes in modes 1 and 2 need 2^22 genes or more: tests/test_gpu_wide_ids.py builds such sets,
almost all of their genes shorter than k.)"""
import numpy as np
import pytest

from tests import helpers as H
from tests import range_stage_sets as R

pytestmark = pytest.mark.gpu


def _assert_counters(cost, c, label):
    assert (cost.groups, cost.shared_records, cost.dictionary_records) == (*R.shared_groups(c), len(c.dictionary)), label


@pytest.mark.parametrize("name", R.SETS)
def test_the_whole_build(name):
    from tests.test_gpu_query import _native
    c = R.case(name)
    nat = _native(c.k, *c.arrays)
    assert nat.cost.total_cost == c.total_cost
    _assert_counters(nat.cost, c, name)
    for g in range(c.genomes):
        H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), c.want[g], f"{name} genome {g}")
    assert [nat.genome_cost(g) for g in range(c.genomes)] == c.genome_cost           # packed ranges: the cost pass on demand
    cost, kl = nat.sequence_costs()
    assert np.array_equal(cost, c.total_visited) and np.array_equal(kl, c.kseq)
    nat.close()


@pytest.mark.parametrize("low_memory", [0, 1])
@pytest.mark.parametrize("name", R.SETS)
def test_genome_batches_of_one(name, low_memory):
    """the build for genome 0, then the ranges again for every further genome; the lonely genome's batch has none"""
    from pandelos_amd.pangene_native import PangeneNative
    c = R.case(name)
    nat = PangeneNative.open()
    costs = []
    for g, s in nat.scores_in_batches(c.k, *c.arrays, 1, low_memory=bool(low_memory)):
        H.assert_scores_equal(s.as_dict(), c.want[g], f"{name} batches of one, low_memory {low_memory}, genome {g}")
        costs.append(nat.genome_cost(g))
        if g == 0:
            _assert_counters(nat.cost, c, name)
            assert nat.cost.total_cost == c.genome_cost[0]                               # a shard reports the lookups of its genomes
    assert costs == c.genome_cost and sum(costs) == c.total_cost
    nat.close()


@pytest.mark.parametrize("ranges,weights", [("sender", True), ("owner", True), ("owner", False)])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", R.SETS)
def test_ranks_together(name, world, ranges, weights):
    from tests.test_gpu_dist import _local
    c = R.case(name)
    label = f"{name} W={world} {ranges} ranges, weights exchanged {weights}"
    lr, cost = _local(world, *c.arrays, c.k, exchange_weights=weights, sender_ranges=ranges == "sender")
    assert lr.used_sender_ranges == (ranges == "sender"), label
    assert lr.total_cost == c.total_cost, label
    assert [lr.genome_cost(g) for g in range(c.genomes)] == c.genome_cost, label
    for n in lr.ranks:                                   # counters over the whole dictionary: the same on every rank
        _assert_counters(n.cost, c, label)
    if world == 3:                                       # one genome per rank / a rank without a genome
        assert sorted(np.bincount(lr.owner, minlength=world).tolist()) == ([1, 1, 1] if c.genomes == 3 else [0, 1, 1]), label
    lr.score_all()
    for g in range(c.genomes):
        H.assert_scores_equal(lr.generate_scores_part(g).as_dict(), c.want[g], f"{label} genome {g}")
    lr.close()


@pytest.mark.parametrize("name", R.SETS)
def test_only_complexity(name):
    from pandelos_amd.pangene_native import PangeneNative
    c = R.case(name)
    nat = PangeneNative.from_arrays(c.k, *c.arrays, only_complexity=True)
    assert nat.cost.total_cost == c.total_cost
    _assert_counters(nat.cost, c, name)
    assert [nat.genome_cost(g) for g in range(c.genomes)] == c.genome_cost
    cost, kl = nat.sequence_costs()
    assert np.array_equal(cost, c.total_visited) and np.array_equal(kl, c.kseq)
    nat.close()
