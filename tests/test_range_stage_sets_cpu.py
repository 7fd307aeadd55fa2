"""The sets of tests/range_stage_sets.py are what tests/test_gpu_range_stage.py takes them for — asserted from the CPU oracle."""
import numpy as np

from tests import helpers as H
from tests import range_stage_sets as R


def test_sets_are_small():
    for name in R.SETS:
        c = R.case(name)
        lengths = np.diff(c.gs.offsets.astype(np.int64))
        assert c.gs.genes <= 40 and lengths.min() >= 30 and lengths.max() <= 100, name


def test_the_lonely_genome_has_no_lookup_and_every_other_gene_has():
    c = R.case("lonely_genome")
    assert c.genomes == 3
    x = R.lonely_gene(c)
    others = np.delete(np.arange(c.gs.genes), x)
    assert c.total_visited[x] == 0 and c.genome_cost[R.LONELY_GENOME] == 0
    assert (c.total_visited[others] > 0).all()
    assert int(c.want[R.LONELY_GENOME]["scoresCount"]) == 0
    # its records are neither the last nor the next-to-last of the dictionary: the fold of the last record does not reach them
    r = H.rank_groups(c.dictionary)[0]
    assert x not in r["seq"][-2:].tolist()
    own = np.flatnonzero(r["seq"] == x)
    assert 0 < own.min() and own.max() < len(r) - 2
    groups, shared = R.shared_groups(c)
    assert groups > 10 and shared > 2 * groups - 1


def test_one_range_is_one_group_of_two_records_at_the_end_of_the_dictionary():
    c = R.case("one_range")
    assert c.genomes == 2 and c.gs.genes == 2
    r, gid, start, sizes = H.rank_groups(c.dictionary)
    assert R.shared_groups(c) == (1, 2)
    assert sizes[-1] == 2 and (sizes[:-1] == 1).all()                        # the shared k-mer is the largest rank: no fold
    assert r["seq"][-2:].tolist() == [0, 1] and r["rank"][-1] == r["rank"][-2]
    assert (r["count"] == 1).all()                                           # "everything else distinct", inside a gene too
    # (one k-mer of forty is too little for a cell: what tells here are the costs and counters, and blocks that stay empty)
    assert c.total_visited.tolist() == [2, 2] and c.total_cost == 4 and c.genome_cost == [2, 2]
