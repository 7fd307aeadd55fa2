"""The group passes (pandelos_amd/csrc/pdl_groups.h) on ONE rank-group of more than 64 tiles of 1024 records: the write side
then finds the borders of a tile's groups more than 64 tiles away (gt_tile_borders past its first look), the costs kernel
walks find_head_back / find_head_fwd past 64 records, and k_gene_costs_lazy scans more than a thousand empty words.
Everything is compared with the CPU oracle (oracle/pangene_oracle.c).

The set: genes of length k = 4, one k-mer each.  70 000 genes are "MMMM" (the big group); in front of it a few singletons
and small groups over the letters A, C (the group neither starts at record 0 nor on a tile border); behind it 1100 groups
of two over the letters P..Y (more than two tiles: the tile the big group ends in looks back past 64 tiles without a head).
Genome 0 holds a single gene of the big group and comes first: its Scores block is one row of about 70 000 cells.

That block is compared in the runs that shard the genomes.  The default build scores all genomes in one symmetric pass, and
a group of more than 65 536 records has more than 2^31 pairs, each stored twice there: more cells than the library takes on
one device (PDL_ERR_UNSUPPORTED), so that run compares the costs only."""
import functools
import itertools

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

K = 4
BIG = 70_000
TILE = 1024


@functools.lru_cache(maxsize=None)
def _set(interleaved: bool):
    """-> (residues, offsets, genome_of).  Gene 0 = genome 0's only gene; the other genes go to genomes 1..4, a genome's
    genes consecutive, or (interleaved) genes 1 and 3 to genome 1 and the rest dealt round-robin over genomes 2..4."""
    front = [b"AAAA", b"AAAC", b"AACA", b"AACA", b"ACAA", b"ACAA", b"ACAA", b"CCCC", b"CCCC"]      # 2 singletons, groups of 2, 3, 2
    after = [bytes(t) for t in itertools.islice(itertools.product(b"PQRSTVWY", repeat=K), 1100)]
    rest = front + [b"MMMM"] * (BIG - 1) + [kmer for kmer in after for _ in range(2)]
    order = np.random.default_rng(7).permutation(len(rest))                     # gene order says nothing about rank order
    genes = [b"MMMM"] + [rest[i] for i in order]
    n = len(genes)
    residues = np.frombuffer(b"".join(genes), np.uint8)
    offsets = np.arange(n + 1, dtype=np.uint64) * K
    if interleaved:
        genome_of = np.concatenate([[0, 1, 2, 1], 2 + np.arange(n - 4) % 3]).astype(np.uint32)
    else:
        genome_of = np.concatenate([[0], 1 + np.arange(n - 1) * 4 // (n - 1)]).astype(np.uint32)
    return residues, offsets, genome_of


@functools.lru_cache(maxsize=None)
def _oracle(interleaved: bool, only_complexity: bool = False):
    from oracle import binding as ob
    ora = ob.Oracle(*_set(interleaved), K, only_complexity=only_complexity)
    if not only_complexity:                               # the set is what the module's docstring says it is
        rank = ora.dictionary()["rank"]
        ranks, sizes = np.unique(rank, return_counts=True)
        big = np.flatnonzero(rank == ranks[np.argmax(sizes)])
        start, size = int(big[0]), len(big)
        assert size == BIG > 64 * TILE and np.array_equal(big, start + np.arange(size))
        assert start > 0 and start % TILE != 0 and len(rank) - (start + size) >= 2 * TILE
    return ora


def _check(nat, ora, genomes, genes, scores=True):
    """total cost, the genomes' costs, per-gene costs of `genes` (None: all) and genome 0's Scores block against the oracle"""
    assert nat.cost.total_cost == sum(ora.genome_cost(g) for g in genomes)
    for g in genomes:
        assert nat.genome_cost(g) == ora.genome_cost(g), g
    cost, kl = nat.sequence_costs()
    sel = slice(None) if genes is None else genes
    assert np.array_equal(cost[sel], ora.total_visited()[sel]) and np.array_equal(kl, ora.kseq_lengths())
    if scores:
        H.assert_scores_equal(nat.generate_scores_part(0).as_dict(), ora.scores(0), "genome 0")


def test_default_build_counts_with_the_histogram_and_files_by_digit():
    """k_range_count_hist + k_range_scatter; the per-gene costs come from k_gene_costs_lazy."""
    from pandelos_amd.pangene_native import PangeneNative
    ora = _oracle(False)
    nat = PangeneNative.from_arrays(K, *_set(False))
    assert nat.cost.total_cost == ora.total_cost
    _check(nat, ora, range(ora.genomes), None, scores=False)


@pytest.mark.parametrize("interleaved,shard", [(False, [0]), (True, [0]), (True, [0, 1])],
                         ids=["consecutive-intervals", "interleaved-one-gene-genome", "interleaved-byte-table"])
def test_shard_before_preprocess_writes_whole_groups_in_record_order(interleaved, shard):
    """Mode 0: k_range_count<0> + k_group_write<0> with 16-byte tuples.  A genome of one gene is one gene-id interval however
    the ids of the others are dealt, so the byte table (GroupTileArgs::in_shard) is reached by adding genome 1, whose two genes
    are not neighbours."""
    from pandelos_amd.pangene_native import PangeneNative
    ora = _oracle(interleaved)
    nat = PangeneNative.open()
    nat.set_genome_shard(shard)
    nat.preprocess(K, *_set(interleaved))
    _check(nat, ora, shard, np.flatnonzero(np.isin(_set(interleaved)[2], shard)))


def test_complexity_only_walks_the_records_around_a_tile():
    """k_group_costs<false, true>: find_head_back / find_head_fwd go past 64 records of one group."""
    from pandelos_amd.pangene_native import PangeneNative
    ora = _oracle(False, True)
    nat = PangeneNative.from_arrays(K, *_set(False), only_complexity=True)
    assert nat.cost.total_cost == ora.total_cost
    assert [nat.genome_cost(g) for g in range(ora.genomes)] == [ora.genome_cost(g) for g in range(ora.genomes)]
