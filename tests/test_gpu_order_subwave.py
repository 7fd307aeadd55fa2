"""K-order with several short rows per wave (option "order_subwave": 1 = the default width, 16 | 32 = lanes per row, 0 = a wave per
row) and the wide rows' workgroups in the same launch (option "order_wide_merged" 1 | 0).

A wave of k_order_rows_sub<W> takes 64 / W task rows, each in a segment of W lanes that holds up to 4 W cells; a row of more cells,
up to 256, is ranked by the whole wave afterwards, a row of more than 256 by the workgroups behind the short rows' ones.
k_mirror_cells_sub gives a source row W lanes.  The rank counts the same keys as before, so every setting must give the CPU
oracle's blocks in emission order, bit for bit, and the blocks of setting 0.

The sets: families of n identical genes of one letter, one gene per genome in genomes 0 .. n-1, at k = 3: every member's row has
n - 1 cells — all its own for the member in genome 0 (every column lies above it), all mirrored for the member in genome n - 1.
The cell counts are 0, 1, W-1, W, W+1 for both widths, 63, 64, 65 (a segment of 16 lanes is full), 127, 128, 129 (one of 32),
255, 256, 257 (a wave is full).  Genome 0 holds a member of every family, in an order that puts rows of different counts into one
wave and a row without cells between two full ones."""
import functools

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

K = 3
CELLS = [256, 0, 257, 1, 15, 255, 16, 64, 0, 63, 17, 31, 65, 32, 33, 127, 0, 128, 129]         # cells of the rows of genome 0, in row order
SMALL = [64, 0, 16, 1, 65, 17, 33]
SETTINGS = [(1, 1), (16, 1), (32, 1), (16, 0), (32, 0)]                                          # (order_subwave, order_wide_merged)
CELL_FIELDS = ("scores", "percs", "tr_percs", "row", "column", "first_seq_genome", "second_seq_genome")


def _family_set(cells):
    """one family per entry of `cells` (n = cells + 1 members, genomes 0 .. n-1), each of a letter of its own"""
    assert len(cells) <= len(H.LETTERS)
    genomes = max(cells) + 1
    genes, gen, fam = [], [], []
    for g in range(genomes):
        for f, c in enumerate(cells):
            if g <= c:
                genes.append(np.repeat(H.LETTERS[f], 5)); gen.append(g); fam.append(f)
    return H._as_gene_set(genes, gen, fam)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The set and the oracle's answer; made once, never changed."""
    cells = CELLS if name == "borders" else SMALL
    c = H.OracleCase(_family_set(cells), K)
    rows = np.concatenate([np.asarray(w["row"], np.int64) for w in c.want])
    cols = np.concatenate([np.asarray(w["column"], np.int64) for w in c.want])
    per_row = np.bincount(rows, minlength=len(c.gs.genome_of))
    assert list(per_row[:len(cells)]) == cells                         # genome 0: the counts asked for, in row order
    own = np.bincount(rows[cols > rows], minlength=len(per_row))
    first_full = cells.index(max(cells))
    assert own[first_full] == per_row[first_full] == max(cells)        # the lowest gene of a family: every cell its own
    assert per_row[-1] == max(cells) and own[-1] == 0                  # the highest: every cell mirrored
    return c


def _open(options, flags=0):
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.open(flags=flags)
    for name, v in options:
        nat.set_option(name, v)
    return nat


def _options(sub, merged):
    return [("order_subwave", sub), ("order_wide_merged", merged)]


def _blocks(nat, genomes):
    return [nat.generate_scores_part(g).as_dict() for g in range(genomes)]


@functools.lru_cache(maxsize=None)
def _parent_blocks(name):
    """what option 0 (a wave per row, k_order_rows behind it) gives; made once, never changed"""
    c = _case(name)
    nat = _open([("order_subwave", 0)])
    nat.preprocess(c.k, *c.arrays)
    blocks = _blocks(nat, c.genomes)
    nat.close()
    for g in range(c.genomes):
        H.assert_scores_equal(blocks[g], c.want[g], f"{name}, order_subwave 0, genome {g}")
    return blocks


def _check(blocks, c, name, label):
    for g in range(c.genomes):
        H.assert_scores_equal(blocks[g], c.want[g], f"{label} genome {g} against the oracle")
        H.assert_scores_equal(blocks[g], _parent_blocks(name)[g], f"{label} genome {g} against order_subwave 0")


@pytest.mark.parametrize("sub,merged", SETTINGS)
def test_rows_at_the_borders_of_a_segment_and_a_wave(sub, merged):
    c = _case("borders")
    nat = _open(_options(sub, merged))
    nat.preprocess(c.k, *c.arrays)
    assert nat.cost.total_cost == c.total_cost
    _check(_blocks(nat, c.genomes), c, "borders", f"order_subwave {sub}, merged {merged}")
    nat.close()


@pytest.mark.parametrize("sub,merged", SETTINGS)
def test_the_same_context_twice_and_after_a_repeated_pass(sub, merged):
    c = _case("small")
    label = f"order_subwave {sub}, merged {merged}"
    nat = _open(_options(sub, merged))
    nat.preprocess(c.k, *c.arrays)
    _check(_blocks(nat, c.genomes), c, "small", label + ", first build")
    one_pass = nat.timings()["join_launches"]
    nat.set_option("staging_cap", 16)                    # far below the cells of one row: the pass overflows and runs again
    nat.preprocess(c.k, *c.arrays)
    _check(_blocks(nat, c.genomes), c, "small", label + ", second build, tiny staging")
    assert nat.timings()["join_launches"] > one_pass     # (a pass queues the tiers once: more than one pass ran)
    nat.close()


@pytest.mark.parametrize("sub,merged", [(0, 1)] + SETTINGS)
def test_without_the_mirror(sub, merged):
    """A genome shard set before the build, then batches of genomes: whole range lists, no mirrored cell, k_mirror_cells not run."""
    c = _case("small")
    label = f"order_subwave {sub}, merged {merged}, no mirror"
    shard = [0, 2, c.genomes - 1]
    nat = _open(_options(sub, merged))
    nat.set_genome_shard(shard)
    nat.preprocess(c.k, *c.arrays)
    for g in shard:
        H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), c.want[g], f"{label}, shard, genome {g}")
    nat.close()
    nat = _open(_options(sub, merged))
    seen = 0
    for g, s in nat.scores_in_batches(c.k, *c.arrays, 24):
        H.assert_scores_equal(s.as_dict(), c.want[g], f"{label}, batches, genome {g}")
        seen += 1
    assert seen == c.genomes
    nat.close()


def _by_column(block):
    """an oracle block as PDL_FLAG_CANONICAL_ORDER gives it: the cells of a row by ascending column"""
    o = np.argsort((np.asarray(block["row"], np.int64) << 32) | np.asarray(block["column"], np.int64), kind="stable")
    return {f: (np.asarray(v)[o] if f in CELL_FIELDS else v) for f, v in block.items()}


@pytest.mark.parametrize("sub,merged", [(0, 1)] + SETTINGS)
def test_canonical_order(sub, merged):
    from pandelos_amd import _lib
    c = _case("borders")
    nat = _open(_options(sub, merged), flags=_lib.PDL_FLAG_CANONICAL_ORDER)
    nat.preprocess(c.k, *c.arrays)
    for g in range(c.genomes):
        H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), _by_column(c.want[g]), f"canonical, order_subwave {sub}, merged {merged}, genome {g}")
    nat.close()


@pytest.mark.parametrize("ranges", ["sender", "owner"])
@pytest.mark.parametrize("sub,merged", [(0, 1), (1, 1), (32, 0)])
def test_an_inbox_behind_the_mirror_kernel(sub, merged, ranges):
    """Two ranks: pdl_dist_score_finish goes through the same score_order as a single GPU's pass — k_mirror_cells(_sub) over the
    rank's own staged cells, then k_mirror_cells_inbox over the received ones, then launch_order."""
    from pandelos_amd.distributed import LocalRanks
    from tests.test_gpu_dist import _device_inputs
    c = _case("small")
    label = f"W=2, {ranges} ranges, order_subwave {sub}, merged {merged}"
    lr = LocalRanks(2, sender_ranges=ranges == "sender")
    for nat in lr.ranks:
        for name, v in _options(sub, merged):
            nat.set_option(name, v)
    lr.preprocess(c.k, *_device_inputs(*c.arrays), len(c.gs.genome_of), len(c.gs.residues))
    assert lr.total_cost == c.total_cost, label
    lr.score_all()
    assert int(lr.outbox_counts.sum()) > 0, label        # cells travelled: the inbox kernel ran
    for g in range(c.genomes):
        H.assert_scores_equal(lr.generate_scores_part(g).as_dict(), c.want[g], f"{label} genome {g}")
    lr.close()


@functools.lru_cache(maxsize=None)
def _query_case():
    """the small set without genome 1 as the base, genome 1 and genome 3 as queries (rows of 0 to 64 cells)"""
    from tests.test_gpu_query import _split
    c = _case("small")
    res, off, gen = c.arrays
    base, q1 = _split(res, off, gen.astype(np.int64), 1)
    _, q3 = _split(res, off, gen.astype(np.int64), 3)
    return base, q1, q3


@pytest.mark.parametrize("sub,merged", [(0, 1)] + SETTINGS)
def test_a_query_and_a_batch_of_three(sub, merged):
    """q_order_rows goes through launch_order too"""
    from tests.test_gpu_query import _check_against_oracle
    base, q1, q3 = _query_case()
    label = f"order_subwave {sub}, merged {merged}"
    nat = _open(_options(sub, merged))
    nat.preprocess(K, *base)
    got1, _ = _check_against_oracle(nat, base, q1, K, label + ", query of genome 1")
    got3, _ = _check_against_oracle(nat, base, q3, K, label + ", query of genome 3")
    assert int(np.bincount(np.asarray(got1["row"])).max()) >= 63
    blocks = nat.query_batch([q1, q3, q1])
    for j, want in enumerate((got1, got3, got1)):
        H.assert_scores_equal(blocks[j].as_dict(), want, f"{label}, batch member {j}")
    nat.close()


@pytest.mark.parametrize("sub,merged", [(0, 1)] + SETTINGS)
def test_a_query_with_a_wide_row(sub, merged):
    """a row of more than 8192 cells: the wide rows' workgroups have work, merged into the launch or behind it"""
    from tests.test_query_golden import assert_block, load_case
    fx, base, query, k, G = load_case("wide_row_9000_columns")
    nat = _open(_options(sub, merged))
    nat.preprocess(k, *base.flatten())
    got = nat.query_idata(query).as_dict()
    assert_block(got, fx, f"wide row, order_subwave {sub}, merged {merged}")
    assert int(np.bincount(np.asarray(got["row"])).max()) > 8192
    q = query.flatten()[:2]
    for block in nat.query_batch([q, q]):
        assert_block(block.as_dict(), fx, f"wide row in a batch, order_subwave {sub}, merged {merged}")
    nat.close()
