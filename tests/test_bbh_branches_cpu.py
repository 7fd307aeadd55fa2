"""The best-hit filter's three host forms on sets that reach every branch of it (CPU oracle only; tests/bbh_sets.py).

Why this file exists.  The filter's forms were compared on the five sets of tests/test_host_net.py::CASES alone.  Three of those
sets hold no intra-genome cell and nothing but best hits among their inter-genome cells, and the five together cannot tell the
filter of Pangenes.java:98-176 from three wrong ones:
  * the test `score < 1.0` in front of inter_max_score (:116) removed          (bbh_sets variant "no_below_1"),
  * the same test widened to `<= 1`                                            ("at_most_1"),
  * phase 2 without the column gene's own best inside the genome (:169)        ("p2_no_column_best");
`>=` against `>` at :170 rested on two cells of one set, and a genome toward which every best hit is 1.0 (inter_max_score 0, row
threshold 0) occurred in none.  (Stated, not asserted: CASES may grow.)

Here: floors on how often each branch is taken in the sets of bbh_sets.SETS — conditions on the sets, not measurements; every
altered filter of bbh_sets.VARIANTS gives another answer than the filter, per set and inside each block that has to stand alone (a
query, a one-genome shard); the restatement bbh_sets.filter_cells, the array form pangenes.bbh_edges (the GPU tests' reference)
and the loop form oracle.pangenes_host.process_genome agree on the sets and on made-up blocks full of ties."""
import numpy as np
import pytest

from pandelos_amd import pangenes as PH
from pandelos_amd.scores import Scores
from tests import bbh_sets as B
from tests import helpers as H

GENERAL = ("chains", "single", "batch")               # sets that carry every event of B.FLOORS


def _as_scores(block):
    return Scores(**{f: block[f] for f in ("scoresCount",) + H.FIELDS})


class _Recorder:
    """Stands in for PangeneNet: the connections in the order process_genome adds them."""
    def __init__(self):
        self.src, self.dst, self.score = [], [], []

    def add_connection(self, src, dest, score):
        self.src.append(src); self.dst.append(dest); self.score.append(score)


def assert_three_forms_agree(block, genomes, sequences, label):
    src, dst, sc = B.edges_of_cells(block, B.filter_cells(block))
    a_src, a_dst, a_sc = PH.bbh_edges(_as_scores(block))
    assert np.array_equal(src, a_src) and np.array_equal(dst, a_dst), f"{label}: filter_cells and bbh_edges name other edges"
    assert H.raw(sc).tobytes() == H.raw(a_sc).tobytes(), f"{label}: filter_cells and bbh_edges differ in a score's bits"
    from oracle import pangenes_host as oh
    rec = _Recorder()
    oh.process_genome(rec, block, genomes, sequences)
    assert rec.src == src.tolist() and rec.dst == dst.tolist(), f"{label}: filter_cells and process_genome name other edges"
    assert H.raw(np.asarray(rec.score, np.float32)).tobytes() == H.raw(sc).tobytes(), f"{label}: process_genome differs in a score's bits"


# ---- the sets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(B.SETS))
def test_sets_stay_small(name):
    gs = B.gene_set(name)
    assert gs.genomes == len(B.SETS[name]["genome_seeds"])
    assert gs.genes <= B.MAX_GENES and sum(int(b["scoresCount"]) for b in B.blocks(name)) <= B.MAX_CELLS


def test_single_is_batch_without_its_last_genome():
    a, b = B.gene_set("single"), B.subset(B.gene_set("batch"), [0, 1, 2, 3])
    assert a.residues.tobytes() == b.residues.tobytes() and np.array_equal(a.offsets, b.offsets) and np.array_equal(a.genome_of, b.genome_of)


def _assert_floors(ev, floors, label):
    short = {e: (ev[e], f) for e, f in floors.items() if ev[e] < f}
    assert not short, f"{label}: (count, floor) {short}"


@pytest.mark.parametrize("name", GENERAL)
def test_floors_of_the_general_sets(name):
    _assert_floors(B.sum_events(B.blocks(name)), B.FLOORS, name)


@pytest.mark.parametrize("name", sorted(B.ALL_BRANCHES))
def test_floors_inside_one_genomes_block(name):
    for label, block in B.all_branch_blocks(name):
        _assert_floors(B.events(block), B.FLOORS, label)


def test_floors_of_the_identical_orthologs():
    blks = B.blocks("identical2")
    ev = B.sum_events(blks)
    _assert_floors(ev, B.FLOORS_IDENTICAL2, "identical2")
    assert ev["best_hits"] == ev["best_hits_at_1"] > 0                 # inter_max_score stays 0 toward both genomes
    assert ev["mutual_kept"] == ev["mutual_kept_thr_0"] and ev["mutual_dropped_below_thr"] == 0


@pytest.mark.parametrize("name", GENERAL)
def test_every_variant_is_killed_by_the_set(name):
    alive = [v for v, where in B.killed_by(B.blocks(name)).items() if not where]
    assert not alive, f"{name}: these altered filters give the filter's cells on every block: {alive}"


@pytest.mark.parametrize("name", sorted(B.ALL_BRANCHES))
def test_every_variant_is_killed_inside_one_genomes_block(name):
    for label, block in B.all_branch_blocks(name):
        alive = [v for v, where in B.killed_by([block]).items() if not where]
        assert not alive, f"{label}: these altered filters give the filter's cells: {alive}"


def test_identical_orthologs_kill_the_variants_of_the_test_below_1():
    where = B.killed_by(B.blocks("identical2"))
    alive = [v for v in ("no_below_1", "at_most_1", "thr_default_0", "no_threshold") if not where[v]]
    assert not alive, alive


# ---- three forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(B.SETS))
def test_three_forms_agree_on_the_sets(name):
    from oracle import pangenes_host as oh
    gs, blks = B.gene_set(name), B.blocks(name)
    parts = []
    for g, block in enumerate(blks):
        assert_three_forms_agree(block, gs.genomes, gs.genes, f"{name} genome {g}")
        parts.append(B.edges_of_cells(block, B.filter_cells(block)))
    text = PH.net_lines(*(np.concatenate([p[i] for p in parts]) for i in range(3)))
    assert text == oh.build_net(lambda g: blks[g], gs.genomes, gs.genes), f"{name}: .net of filter_cells against build_net"

    class _Native:
        def generate_scores_part(self, g, multithread=False):
            return _as_scores(blks[g])
    assert PH.run(_Native(), gs.genomes) == text, f"{name}: .net of pangenes.run"


SCORE_VALUES = np.array([0.25, 0.5, 0.75, 1.0], np.float32)


def made_up_block(seed):
    """A Scores block that comes from no gene set: 2-5 genomes of 1-6 genes, the rows of one of them against random columns, scores
    from SCORE_VALUES (ties, 1.0 and cells at the threshold are the rule), the three tables made from the cells as the native side
    makes them: scoresMaxMappings = a row gene's place among its genome's genes and INT32_MAX elsewhere, max_genome_score[row][genome]
    and max_genome_score_col[column] the largest score of the block's cells there, 0 without one.  Every second block mirrors its
    intra-genome cells, every third has its cells in no order.  -> (block, genomes, sequences)"""
    rng = np.random.default_rng(50_000 + seed)
    G = int(rng.integers(2, 6))
    genome_of = np.repeat(np.arange(G), rng.integers(1, 7, G))
    N, g = len(genome_of), int(rng.integers(0, G))
    rows = np.nonzero(genome_of == g)[0]
    density = (0.0, 0.3, 0.6, 0.9)[int(rng.integers(0, 4))] if seed % 10 else 0.0
    cells = {}
    for r in rows:
        for c in rng.permutation(N):
            if c != r and rng.random() < density:
                cells[int(r), int(c)] = SCORE_VALUES[int(rng.integers(0, 4))]
    if seed % 2 == 0:
        for (r, c), v in list(cells.items()):
            if genome_of[c] == g and r < c:
                cells[c, r] = v
    keys = list(cells)
    if seed % 3 == 0:
        keys = [keys[i] for i in rng.permutation(len(keys))]
    row = np.array([r for r, _ in keys], np.int32)
    col = np.array([c for _, c in keys], np.int32)
    score = np.array([cells[key] for key in keys], np.float32)
    at = np.full(N, B.INT32_MAX, np.int32)
    at[rows] = np.arange(len(rows), dtype=np.int32)
    best, col_best = np.zeros((len(rows), G), np.float32), np.zeros(N, np.float32)
    if len(keys):
        np.maximum.at(best, (at[row], genome_of[col]), score)
        np.maximum.at(col_best, col, score)
    block = {"scoresCount": len(keys), "scores": score, "percs": score.copy(), "tr_percs": score.copy(), "row": row, "column": col,
             "first_seq_genome": genome_of[row].astype(np.int32), "second_seq_genome": genome_of[col].astype(np.int32),
             "max_genome_score": best, "max_genome_score_col": col_best, "scoresMaxMappings": at}
    return block, G, N


def test_three_forms_agree_on_made_up_blocks():
    seen = dict.fromkeys(B.EVENTS, 0)
    for seed in range(300):
        block, G, N = made_up_block(seed)
        assert_three_forms_agree(block, G, N, f"made-up block {seed}")
        for e, v in B.events(block).items():
            seen[e] += v
    _assert_floors(seen, {e: 10 for e in B.EVENTS}, "the made-up blocks together")       # dense in every event, ties above all


def test_made_up_blocks_kill_every_variant():
    blks = [made_up_block(seed)[0] for seed in range(300)]
    alive = [v for v, where in B.killed_by(blks).items() if not where]
    assert not alive, alive
