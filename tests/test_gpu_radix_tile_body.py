"""The radix tile body (pdl_sort.h: ranking, tile layout, placement, write-out) that k_rs_scatter and k_range_scatter share.

Driven as test_gpu_radix_launches.py drives its cases: a build through the public entry points under option "lean_radix" 1 and
0, the dictionary stage against the CPU oracle (records in the oracle's order, per-gene lookups and k-mer counts, groups,
shared records, total cost) and, for the small sets, every genome's Scores block bit for bit.  Every set has fewer ranges than
records (asserted: a group's last member gets no range), so the gene sort's passes behind the range scatter run on a device-side
count below the bound their grids are sized for.

What the sets are for:
  rank width k      two letters, k = 1 .. 16: ranks of k bits, the rank sort's last pass matches 1 .. 8 bits — as its only pass
                    (k <= 8) and behind a full first one (k > 8); about 5 000 k-mers, two tiles
  gene width N      N genes of 8-12 residues at k = 3: the gene sort's pass behind the range scatter matches 1 .. 8 bits
                    (N = 257 .. 65 536), there is none (N <= 256), a third of 1 bit (N > 65 536)
  one digit         a gene of 9 000 identical residues: whole rounds and whole tiles of one digit, ranks inside a tile up to
                    4095 in their 16-bit field, one counter taking every count of a wave
  distinct digits   any 64 consecutive k-mers of the stream differ in the low byte of their rank: every lane is the first of
                    its digit in every round of the first pass
  short:M           M = 1 .. 257 k-mers: tiles of less than a wave, a wave and one element, less than a round of the workgroup
  64-bit keys       a k = 13 fixture"""
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests.test_gpu_radix_launches import _Want, _assert_dictionary_stage, _open

pytestmark = pytest.mark.gpu

LEAN = [1, 0]
RANK_K = list(range(1, 17))
GENE_N = [2, 255, 256, 257, 300, 700, 1500, 3000, 6000, 12000, 24000, 40000, 65536, 65537, 70000]
GENE_N_SCORED = 6000                                     # above: the dictionary stage only (the oracle's scoring is what takes long there)
SHORT_M = [1, 63, 64, 65, 255, 257]


def _two_letter_set(k: int):
    """3 genomes, genes of 40-80 residues over two letters, dealt in turn until there are just over 5 000 k-mers"""
    rng = np.random.default_rng(1000 + k)
    genes, gen, m = [], [], 0
    while m < 5000:
        ln = int(rng.integers(40, 81))
        genes.append(H.LETTERS[rng.integers(0, 2, ln)]); gen.append(len(genes) % 3)
        m += ln - k + 1
    order = np.argsort(gen, kind="stable")
    return H._as_gene_set([genes[i] for i in order], [gen[i] for i in order], [-1] * len(genes))


def _short_gene_set(n: int):
    """n genes of 8-12 residues in 3 genomes (2 when there are only two genes)"""
    rng = np.random.default_rng(2000 + n)
    genomes = min(3, n)
    genes = [H.LETTERS[rng.integers(0, 20, int(rng.integers(8, 13)))] for _ in range(n)]
    gen = [i * genomes // n for i in range(n)]
    return H._as_gene_set(genes, gen, [-1] * n)


def _one_digit_set():
    rng = np.random.default_rng(81)
    genes, gen = [], []
    for g in range(3):
        for i in range(40):
            if g == 1 and i == 7:
                genes.append(np.full(9000, H.LETTERS[5], dtype=np.uint8))
            else:
                genes.append(H.LETTERS[rng.integers(0, 20, int(rng.integers(50, 101)))])
            gen.append(g)
    return H._as_gene_set(genes, gen, [-1] * len(genes))


def _low_bytes(genes, k):
    """low byte of every k-mer's rank, in stream order (all twenty letters occur: a letter's rank value is its place in LETTERS)"""
    out = []
    for g in genes:
        r = np.searchsorted(H.LETTERS, g).astype(np.int64)
        out.append(sum(r[i:len(r) - k + 1 + i] * 20 ** (k - 1 - i) for i in range(k)) & 0xff)
    return np.concatenate(out)


def _distinct_digit_set(k: int = 3):
    """Two genomes of one gene of 2 600 residues each, grown letter by letter so that the new k-mer's low rank byte is none of the
    63 before it in the stream; every letter occurs."""
    rng = np.random.default_rng(82)
    recent, genes = [], []
    for _ in range(2):
        r = [int(x) for x in rng.integers(0, 20, k - 1)]
        while len(r) < 2600:
            head = sum(r[len(r) - (k - 1) + i] * 20 ** (k - 1 - i) for i in range(k - 1))
            free = [c for c in rng.permutation(20) if ((head + int(c)) & 0xff) not in recent[-63:]]
            assert free, "no letter keeps the low bytes apart"
            r.append(int(free[0])); recent.append((head + r[-1]) & 0xff)
        genes.append(H.LETTERS[np.array(r)])
    assert len(np.unique(np.concatenate(genes))) == 20
    return H._as_gene_set(genes, [0, 1], [-1, -1])


def _short_stream_set(m: int, k: int = 3):
    """m k-mers in all, two genomes: genes of at most 40 residues, the first genome gets the larger half; a gene shorter than k
    (no k-mer) closes each genome, so that the second one exists when m = 1"""
    rng = np.random.default_rng(3000 + m)
    genes, gen = [], []
    for g, part in enumerate((m - m // 2, m // 2)):
        while part > 0:
            take = min(40 - k + 1, part)
            genes.append(H.LETTERS[rng.integers(0, 20, take + k - 1)]); gen.append(g)
            part -= take
        genes.append(H.LETTERS[rng.integers(0, 20, k - 1)]); gen.append(g)
    return H._as_gene_set(genes, gen, [-1] * len(genes))


@functools.lru_cache(maxsize=None)
def _case(name):
    kind, _, arg = name.partition(":")
    if kind == "rank_k":
        gs = _two_letter_set(int(arg)); return _Want(gs.residues, gs.offsets, gs.genome_of, int(arg))
    if kind == "gene_n":
        gs = _short_gene_set(int(arg)); return _Want(gs.residues, gs.offsets, gs.genome_of, 3, scores=int(arg) <= GENE_N_SCORED)
    if kind == "one_digit":
        gs = _one_digit_set(); return _Want(gs.residues, gs.offsets, gs.genome_of, 3)
    if kind == "distinct":
        gs = _distinct_digit_set(); return _Want(gs.residues, gs.offsets, gs.genome_of, 3)
    if kind == "short":
        gs = _short_stream_set(int(arg)); return _Want(gs.residues, gs.offsets, gs.genome_of, 3)
    if kind == "fixture":
        res, off, gen, k, _ = H.load_small(arg); return _Want(res, off, gen, k, scores=False)
    raise KeyError(name)


def _ranges_and_records(w):
    """ranges of the single-GPU build = the records of every rank-group of >= 2 but the group's last (groups as the reference's
    scan forms them, see _assert_dictionary_stage)"""
    d = w.dictionary
    rk = np.sort(d["rank"])
    heads = np.flatnonzero(np.r_[True, rk[1:-1] != rk[:-2]]) if len(d) > 1 else np.array([0])
    sizes = np.diff(np.r_[heads, max(len(d) - 1, 1)]).astype(np.int64)
    if len(d) > 1:
        sizes[-1] += 1
    return int((sizes[sizes >= 2] - 1).sum()), len(d)


def _check(name, lean):
    w = _case(name)
    label = f"{name} lean_radix={lean}"
    ranges, records = _ranges_and_records(w)
    assert ranges < records, label
    nat = _open(w, lean)
    _assert_dictionary_stage(nat, w, label)
    assert nat.cost.shared_records - nat.cost.groups == ranges, label
    if w.scores is not None:
        for g in range(w.genomes):
            H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), w.scores[g], f"{label} genome {g}")
    return w, nat


@pytest.mark.parametrize("lean", LEAN)
@pytest.mark.parametrize("k", RANK_K)
def test_rank_sort_last_pass_of_every_width(k, lean):
    w, nat = _check(f"rank_k:{k}", lean)
    assert nat.cost.rank_bits == k and not nat.cost.hash_fallback
    assert 4096 < w.kmer_occurrences <= 8192             # two tiles
    nat.close()


@pytest.mark.parametrize("lean", LEAN)
@pytest.mark.parametrize("n", GENE_N)
def test_gene_sort_last_pass_of_every_width(n, lean):
    w, nat = _check(f"gene_n:{n}", lean)
    assert nat.cost.sequences == n
    nat.close()


@pytest.mark.parametrize("lean", LEAN)
def test_rounds_and_tiles_of_one_digit(lean):
    w, nat = _check("one_digit", lean)
    assert int(w.kseq.max()) == 9000 - 3 + 1             # more than two tiles of one k-mer
    nat.close()


@pytest.mark.parametrize("lean", LEAN)
def test_rounds_of_sixty_four_different_digits(lean):
    w, nat = _check("distinct", lean)
    res, off, _ = w.arrays
    genes = [np.asarray(res[off[i]:off[i + 1]]) for i in range(len(off) - 1)]
    low = _low_bytes(genes, 3)
    assert nat.cost.rank_base == 20 and len(low) == w.kmer_occurrences > 4096
    for i in range(0, len(low) - 63):
        assert len(set(low[i:i + 64].tolist())) == 64, i
    nat.close()


@pytest.mark.parametrize("lean", LEAN)
@pytest.mark.parametrize("m", SHORT_M)
def test_tiles_of_less_than_a_wave_and_just_over(m, lean):
    w, nat = _check(f"short:{m}", lean)
    assert w.kmer_occurrences == m
    nat.close()


@pytest.mark.parametrize("lean", LEAN)
def test_sixty_four_bit_keys(lean):
    name = "synth_5x60x80_k13"
    w, nat = _check(f"fixture:{name}", lean)
    _, _, _, _, fx = H.load_small(name)
    assert nat.cost.rank_bits > 32 and nat.cost.total_cost == int(fx["total_cost"])
    H.assert_scores_equal_fixture(lambda g: nat.generate_scores_part(g).as_dict(), fx, w.genomes, f"{name} lean_radix={lean}")
    nat.close()
