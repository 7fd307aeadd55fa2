"""The radix passes of the dictionary build with option "lean_radix" 1 (the default) and 0.

"lean_radix" 1: the offsets of a pass come from ONE launch (k_rs_offsets: a workgroup scans the row of one digit; the scatter
kernels add up the 256 digit bases themselves and workgroup 0 writes the grand total), and K-rank works a radix tile of 4096
slots per workgroup and files the rank sort's first histogram (k_rank<KeyT, 2>), so that pass makes none.  0: a k_rs_hist and a
three-launch scan over the whole count table for every pass, K-rank in tiles of 1024.  K-rank's bracket of a tile is a wave-wide
search either way.

Every case, under both values: the dictionary stage equals the CPU oracle — rank table, (rank, gene, count) records in the
oracle's order, per-gene lookups and k-mer counts, groups, shared records, total cost (the grand total of the range scatter is
what the gene sort's second pass, the range offsets and the host read as the range count: every set here has fewer ranges than
records, so that pass runs tiles past the end of a device-side count).  Cases with scores also compare every genome's block with
the oracle (or the reference's fixture), bit for bit: a range filed under the wrong gene or at the wrong place changes them.

What the sets are for:
  edge:M        M k-mers exactly, k = 3: one tile short of full (4095), full (4096), a second tile of one element (4097), two
                full tiles (8192), a third of one element (8193) — the row scan with one, two and three entries
  long_rows     311 radix tiles: a row of the count table spans several waves of the scanning workgroup (a thread holds four
                entries) and K-rank's grid has hundreds of workgroups; ranks of 22 bits, so the last pass has 6
  many_genes    over 1000 genes under a K-rank tile (more than RANK_SPAN = 128: boundaries are looked up in global memory), with
                genes shorter than k, which have no k-mer, between them
  giant_gene    one gene of 20 000 residues among genes of 50-100: tiles whose bracket is that one gene, then a tile with many
  two_letters   alphabet of two letters, k = 3: ranks of 3 bits, one pass with 3 significant bits
  fixtures      64-bit keys (k = 13: the histogram comes from k_rank<uint64_t, 2>) and hashed ranks (k = 16: k_rank_hash files
                none, every pass keeps its k_rs_hist)"""
import functools

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

LEAN = [1, 0]
EDGE_M = [4095, 4096, 4097, 8192, 8193]


class _Want:
    """What the oracle says about a set; made once per set, never changed."""

    def __init__(self, res, off, gen, k, scores=True):
        from oracle import binding as ob
        ora = ob.Oracle(res, off, gen, k)
        self.arrays, self.k, self.genomes = (res, off, gen), k, int(ora.genomes)
        self.rank_values, self.last_multiplier = np.array(ora.rank_values), int(ora.last_multiplier)
        self.rank_base, self.kmer_occurrences = int(ora.rank_base), int(ora.kmer_occurrences)
        self.dictionary = np.array(ora.dictionary())
        self.total_visited, self.kseq = np.array(ora.total_visited()), np.array(ora.kseq_lengths())
        self.total_cost = int(ora.total_cost)
        self.scores = [ora.scores(g) for g in range(self.genomes)] if scores else None
        ora.close()


def _edge_set(m_target: int, k: int = 3):
    """Two genomes whose genes have m_target k-mers in all: genes of 100 residues, the last one cut to fit; the second genome's
    genes are copies of the first's with one residue in ten replaced."""
    rng = np.random.default_rng(m_target)
    half = m_target // 2
    lens, n0 = [], 0
    for part in (half, m_target - half):
        left = part
        while left > 0:
            take = min(100 - k + 1, left)
            lens.append(take + k - 1)
            left -= take
        n0 = n0 or len(lens)                             # genes of the first genome
    first = [H.LETTERS[rng.integers(0, 20, 100)] for _ in range(n0)]
    genes, gen = [], []
    for i, ln in enumerate(lens):
        src = first[i % n0].copy()
        if i >= n0:
            hit = rng.random(100) < 0.1
            src[hit] = H.LETTERS[rng.integers(0, 20, int(hit.sum()))]
        genes.append(src[:ln])
        gen.append(0 if i < n0 else 1)
    gs = H._as_gene_set(genes, gen, [-1] * len(genes))
    assert int(sum(max(len(g) - k + 1, 0) for g in genes)) == m_target
    return gs


def _many_genes_set(k: int = 3):
    """3 genomes x 3000 genes of k+1 .. k+2 residues, a gene shorter than k after every one of them"""
    rng = np.random.default_rng(77)
    genes, gen = [], []
    for g in range(3):
        for _ in range(3000):
            genes.append(H.LETTERS[rng.integers(0, 20, k + 1 + int(rng.integers(0, 2)))]); gen.append(g)
            genes.append(H.LETTERS[rng.integers(0, 20, int(rng.integers(1, k)))]); gen.append(g)
    return H._as_gene_set(genes, gen, [-1] * len(genes))


def _giant_gene_set():
    rng = np.random.default_rng(78)
    genes, gen = [], []
    for g in range(3):
        for i in range(60):
            if g == 1 and i == 20:
                genes.append(H.LETTERS[rng.integers(0, 20, 20000)])
            else:
                genes.append(H.LETTERS[rng.integers(0, 20, int(rng.integers(50, 101)))])
            gen.append(g)
    return H._as_gene_set(genes, gen, [-1] * len(genes))


def _two_letter_set():
    rng = np.random.default_rng(79)
    genes, gen = [], []
    for g in range(3):
        for _ in range(40):
            genes.append(H.LETTERS[rng.integers(0, 2, int(rng.integers(20, 60)))]); gen.append(g)
    return H._as_gene_set(genes, gen, [-1] * len(genes))


@functools.lru_cache(maxsize=None)
def _case(name):
    kind, _, arg = name.partition(":")
    if kind == "edge":
        gs = _edge_set(int(arg)); return _Want(gs.residues, gs.offsets, gs.genome_of, 3)
    if kind == "long_rows":
        from pandelos_amd.synth import make_gene_set
        gs = make_gene_set(genomes=3, genes_per_genome=600, mean_len=700, sub_rate=0.2, seed=903)
        return _Want(gs.residues, gs.offsets, gs.genome_of, 5, scores=False)
    if kind == "many_genes":
        gs = _many_genes_set(); return _Want(gs.residues, gs.offsets, gs.genome_of, 3)
    if kind == "giant_gene":
        gs = _giant_gene_set(); return _Want(gs.residues, gs.offsets, gs.genome_of, 3)
    if kind == "two_letters":
        gs = _two_letter_set(); return _Want(gs.residues, gs.offsets, gs.genome_of, 3)
    if kind == "fixture":
        res, off, gen, k, _ = H.load_small(arg); return _Want(res, off, gen, k, scores=False)
    raise KeyError(name)


def _open(want, lean):
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.open()
    nat.set_option("lean_radix", lean)
    nat.preprocess(want.k, *want.arrays)
    return nat


def _assert_dictionary_stage(nat, w, label):
    tab, lm = nat.rank_table()
    assert np.array_equal(tab, w.rank_values) and lm == w.last_multiplier, label
    assert nat.cost.rank_base == w.rank_base and nat.cost.kmer_occurrences == w.kmer_occurrences, label
    ranks, seqs, counts = nat.dictionary()
    d = w.dictionary
    assert np.array_equal(ranks, d["rank"]), f"{label}: ranks"
    assert np.array_equal(seqs, d["seq"]), f"{label}: genes"
    assert np.array_equal(counts, d["count"]), f"{label}: counts"
    cost, kl = nat.sequence_costs()
    assert np.array_equal(cost, w.total_visited), f"{label}: per-gene lookups"
    assert np.array_equal(kl, w.kseq), f"{label}: k-mers per gene"
    # rank-groups of >= 2 records as the reference's scan forms them (the last record never opens one, it joins the group before)
    rk = np.sort(d["rank"])
    heads = np.flatnonzero(np.r_[True, rk[1:-1] != rk[:-2]]) if len(d) > 1 else np.array([0])
    sizes = np.diff(np.r_[heads, max(len(d) - 1, 1)]).astype(np.int64)
    if len(d) > 1:
        sizes[-1] += 1
    assert nat.cost.groups == int((sizes >= 2).sum()), f"{label}: groups"
    assert nat.cost.shared_records == int(sizes[sizes >= 2].sum()), f"{label}: shared records"
    assert nat.cost.total_cost == int((sizes[sizes >= 2] ** 2).sum()) == w.total_cost, f"{label}: total cost"


def _check(name, lean):
    w = _case(name)
    label = f"{name} lean_radix={lean}"
    nat = _open(w, lean)
    _assert_dictionary_stage(nat, w, label)
    if w.scores is not None:
        for g in range(w.genomes):
            H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), w.scores[g], f"{label} genome {g}")
    nat.close()
    return w


@pytest.mark.parametrize("lean", LEAN)
@pytest.mark.parametrize("m", EDGE_M)
def test_tile_edges(m, lean):
    w = _check(f"edge:{m}", lean)
    assert w.kmer_occurrences == m


@pytest.mark.parametrize("lean", LEAN)
def test_rows_of_311_tiles_and_a_last_pass_of_six_bits(lean):
    w = _check("long_rows", lean)
    assert w.kmer_occurrences == 1272633                       # 311 radix tiles
    nat = _open(w, lean)
    assert nat.cost.rank_bits == 22
    nat.close()


@pytest.mark.parametrize("lean", LEAN)
def test_more_genes_under_a_tile_than_k_rank_stages(lean):
    w = _check("many_genes", lean)
    assert int((w.kseq == 0).sum()) >= 9000 and w.kmer_occurrences / 4096 * 128 < int((w.kseq > 0).sum())


@pytest.mark.parametrize("lean", LEAN)
def test_one_gene_across_many_tiles(lean):
    w = _check("giant_gene", lean)
    assert int(w.kseq.max()) == 20000 - 3 + 1


@pytest.mark.parametrize("lean", LEAN)
def test_two_letter_alphabet_sorts_in_one_pass_of_three_bits(lean):
    w = _check("two_letters", lean)
    nat = _open(w, lean)
    assert nat.cost.rank_bits == 3
    nat.close()


@pytest.mark.parametrize("lean", LEAN)
@pytest.mark.parametrize("name", ["synth_5x60x80_k13", "synth_5x60x80_k16_hash"])
def test_wide_and_hashed_keys(name, lean):
    w = _check(f"fixture:{name}", lean)
    _, _, _, _, fx = H.load_small(name)
    nat = _open(w, lean)
    assert nat.cost.total_cost == int(fx["total_cost"])
    assert [nat.genome_cost(g) for g in range(w.genomes)] == [int(x) for x in fx["genome_cost"]]
    H.assert_scores_equal_fixture(lambda g: nat.generate_scores_part(g).as_dict(), fx, w.genomes, f"{name} lean_radix={lean}")
    nat.close()
