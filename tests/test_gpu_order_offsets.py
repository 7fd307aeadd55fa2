"""K-order's cell offsets: fin_off[p] (cells of the task rows before p, own + mirrored), m_off[p] (their mirrored cells) and the
two totals.  With upper-triangle range lists they come from one launch (k_order_offsets in pdl_join.hip, option "order_offsets":
2 = several workgroups, one per 4096 rows; 1 = one workgroup; 0 = two prefix scans) for up to "order_offsets_rows" task rows, from
the scans beyond that and without the mirror.

What a caller sees of them: every row's cells lie at fin_off[row] in its genome's block, the row's own cells first and the mirrored
ones (column below the row) at m_off[row] of the mirrored copies; pdl_scores_counts gives fin_off at the genomes' first rows and the
timings' emitted_cells the total.  So each case compares every block with the CPU oracle field for field, in emission order, and
the offsets read back from the blocks with a numpy cumsum over the oracle's cells.

Row counts: 1, 63, 64, 65, one tile of 4096 rows +- 1, and a bound lowered to 64 rows with 63, 64 and 65 rows; rows without a cell at
the front, in the middle and at the end of the task order.  A library that does not know the two options (the scans alone) passes
the same checks."""
import functools

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

K = 3
GENOMES = 3
TILE = 4096                                              # OO_TILE in pdl_join.hip
LONELY = [np.frombuffer(x, dtype=np.uint8) for x in (b"K", b"L", b"M")]                   # one letter each: genes that share nothing
BODY_LETTERS = np.array([c for c in H.LETTERS if c not in b"KLM"], dtype=np.uint8)       # both ends of the alphabet: the last record is a body's


def _row_set(n, seed=5, sub=0.1):
    """n genes in three genomes, genome by genome (task position = gene id).  With n >= 9 the first, the middle and the last gene
    are runs of one private letter: their k-mer is nobody else's, they get no range and their rows no cell."""
    rng = np.random.default_rng(seed + n)
    fams = max(1, n // GENOMES)
    bases = [BODY_LETTERS[rng.integers(0, len(BODY_LETTERS), int(rng.integers(30, 41)))] for _ in range(fams)]
    lonely = {0: LONELY[0], n // 2: LONELY[1], n - 1: LONELY[2]} if n >= 9 else {}
    genes, gen, fam = [], [], []
    for i in range(n):
        f = i % fams
        if i in lonely:
            genes.append(np.repeat(lonely[i], 35)); fam.append(-1)
        else:
            s = bases[f].copy()
            m = rng.random(len(s)) < sub
            s[m] = BODY_LETTERS[rng.integers(0, len(BODY_LETTERS), int(m.sum()))]
            genes.append(s); fam.append(f)
        gen.append(min(i * GENOMES // n, GENOMES - 1) if n >= GENOMES else i)
    return H._as_gene_set(genes, gen, fam), sorted(lonely)


@functools.lru_cache(maxsize=None)
def _case(n):
    """The set, the oracle's answer and the offsets a numpy cumsum makes of it; made once, never changed."""
    gs, lonely = _row_set(n)
    c = H.OracleCase(gs, K)
    rows = np.concatenate([np.asarray(w["row"], np.int64) for w in c.want])
    cols = np.concatenate([np.asarray(w["column"], np.int64) for w in c.want])
    cells = np.bincount(rows, minlength=n)
    mirrored = np.bincount(rows[cols < rows], minlength=n)           # a row's own lookups reach only the genes above it
    c.fin_off = np.concatenate([[0], np.cumsum(cells)])
    c.m_off = np.concatenate([[0], np.cumsum(mirrored)])
    c.lonely = lonely
    for i in lonely:
        assert cells[i] == 0
    if n >= 9:
        assert c.fin_off[-1] > 0 and c.m_off[-1] * 2 == c.fin_off[-1]     # every cell is there twice: once mirrored
    return c


def _set_options(nat, options):
    """-> False when the library does not know them (it then has the scans alone)"""
    try:
        for name, v in options:
            nat.set_option(name, v)
        return True
    except Exception:
        return False


def _offsets_of_blocks(blocks, n):
    rows = np.concatenate([np.asarray(b["row"], np.int64) for b in blocks])
    cols = np.concatenate([np.asarray(b["column"], np.int64) for b in blocks])
    assert np.all(np.diff(rows) >= 0)                    # task order: a row's cells are contiguous, at fin_off[row]
    fin = np.searchsorted(rows, np.arange(n + 1))        # first cell of every row = cells of the rows before it
    below = cols < rows
    m_off = np.concatenate([[0], np.cumsum(np.bincount(rows[below], minlength=n))])
    return fin, m_off


def _check_single(n, options, label):
    from pandelos_amd.pangene_native import PangeneNative
    c = _case(n)
    nat = PangeneNative.open()
    _set_options(nat, options)
    nat.preprocess(c.k, *c.arrays)
    assert nat.cost.total_cost == c.total_cost, label
    blocks = [nat.generate_scores_part(g).as_dict() for g in range(c.genomes)]
    for g in range(c.genomes):
        H.assert_scores_equal(blocks[g], c.want[g], f"{label} genome {g}")
    fin, m_off = _offsets_of_blocks(blocks, n)
    assert np.array_equal(fin, c.fin_off) and np.array_equal(m_off, c.m_off), label
    firsts = np.searchsorted(c.gs.genome_of, np.arange(c.genomes + 1))          # the genomes' first rows
    assert np.array_equal(np.asarray(nat.scores_counts(), np.int64), np.diff(c.fin_off[firsts])), label
    assert nat.timings()["emitted_cells"] == c.fin_off[-1], label                # the total (and its second copy: fin_off[n])
    nat.close()


FORMS = [2, 1, 0]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_row_counts_around_a_wave_and_a_tile(n, form):
    _check_single(n, [("order_offsets", form)], f"{n} rows, order_offsets {form}")


@pytest.mark.parametrize("form", [2, 1])
@pytest.mark.parametrize("n", [63, 64, 65])
def test_row_counts_around_a_lowered_bound(n, form):
    """64 rows at most for the one launch: 63 and 64 rows take it, 65 the scans"""
    _check_single(n, [("order_offsets", form), ("order_offsets_rows", 64)], f"{n} rows, bound 64, order_offsets {form}")


@pytest.mark.parametrize("n", [2 * TILE + 77])
def test_three_workgroups_and_twelve_trips_of_one(n):
    """the last workgroup adds up two whole parts in front of its own; one workgroup carries its prefix over three trips"""
    for form in (2, 1):
        _check_single(n, [("order_offsets", form)], f"{n} rows, order_offsets {form}")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [65, TILE + 1])
def test_without_the_mirror(n, form):
    """A genome shard set before the build: whole groups for its genes, no mirrored cell, the scans whatever the option says."""
    from pandelos_amd.pangene_native import PangeneNative
    c = _case(n)
    shard = [0, 2]
    nat = PangeneNative.open()
    _set_options(nat, [("order_offsets", form)])
    nat.set_genome_shard(shard)
    nat.preprocess(c.k, *c.arrays)
    blocks = {g: nat.generate_scores_part(g).as_dict() for g in shard}
    for g in shard:
        H.assert_scores_equal(blocks[g], c.want[g], f"{n} rows, shard {shard}, order_offsets {form}, genome {g}")
    counts = np.asarray(nat.scores_counts(), np.int64)
    firsts = np.searchsorted(c.gs.genome_of, np.arange(c.genomes + 1))
    per_genome = np.diff(c.fin_off[firsts])
    assert [int(counts[g]) for g in shard] == [int(per_genome[g]) for g in shard]
    assert nat.timings()["emitted_cells"] == sum(int(per_genome[g]) for g in shard)
    nat.close()


@pytest.mark.parametrize("ranges", ["sender", "owner"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [65, TILE + 1])
def test_an_inbox_adds_mirrored_cells(n, form, ranges):
    """Two ranks: the cells whose column another rank owns arrive in an inbox and are counted into mirror_cnt before the offsets
    are made.  A rank's task rows are the genes of its genomes."""
    from pandelos_amd.distributed import LocalRanks
    from tests.test_gpu_dist import _device_inputs
    c = _case(n)
    label = f"{n} rows, W=2, {ranges} ranges, order_offsets {form}"
    lr = LocalRanks(2, sender_ranges=ranges == "sender")
    for nat in lr.ranks:
        _set_options(nat, [("order_offsets", form)])
    lr.preprocess(c.k, *_device_inputs(*c.arrays), len(c.gs.genome_of), len(c.gs.residues))
    assert lr.total_cost == c.total_cost, label
    lr.score_all()
    assert int(lr.outbox_counts.sum()) > 0, label        # cells travelled
    blocks = [lr.generate_scores_part(g).as_dict() for g in range(c.genomes)]
    for g in range(c.genomes):
        H.assert_scores_equal(blocks[g], c.want[g], f"{label} genome {g}")
    fin, m_off = _offsets_of_blocks(blocks, n)           # (the ranks' offsets laid end to end in genome order)
    assert np.array_equal(fin, c.fin_off) and np.array_equal(m_off, c.m_off), label
    firsts = np.searchsorted(c.gs.genome_of, np.arange(c.genomes + 1))
    per_genome = np.diff(c.fin_off[firsts])
    for r, nat in enumerate(lr.ranks):                   # each rank's total: the cells of its genomes
        assert nat.timings()["emitted_cells"] == sum(int(per_genome[g]) for g in range(c.genomes) if int(lr.owner[g]) == r), label
    lr.close()
