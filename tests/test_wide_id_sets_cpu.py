"""The sets of tests/wide_id_sets.py reach the cases tests/test_gpu_wide_ids.py is about, shown on the CPU oracle alone: gene counts
on both sides of 2^22, cells whose column is wrong once 22 bits of it are kept, rows for every branch of K-order, rank groups and
costs across the limit, and a base under the limit that an appended genome lifts over it.  No device.

A block of genome 0 (4.19 M rows) takes the oracle 12-14 s, so only "above", "lift" and "lift+" fetch theirs here."""
import numpy as np
import pytest

from tests import helpers as H
from tests import wide_id_sets as W

B = W.B


@pytest.mark.parametrize("name", W.SIZES)
def test_gene_count_against_the_limit(name):
    c = W.case(name)
    assert c.genomes == 3 and c.k == 4 and len(c.arrays[2]) == c.n
    assert {"below": c.n == B - 1, "at": c.n == B, "above": B + 1000 < c.n < B + 2000}[name]
    real = c.real
    assert len(real) == 27 + W.REAL_1 + W.REAL_2 and real[-1] == c.n - 1                 # the set's last gene is real
    lens = np.diff(c.arrays[1].astype(np.int64))
    assert (lens[real] == W.GENE_LEN).all() and c.kseq[real].min() > 2 * c.k              # only the missing packed ranges keep tier 0 away
    filler = np.setdiff1d(np.arange(c.n), real)
    assert set(np.unique(lens[filler]).tolist()) == {0, c.k - 1} and 0.2 < (lens[filler] == c.k - 1).mean() < 0.3
    assert (c.kseq[filler] == 0).all() and (c.total_visited[filler] == 0).all()
    assert real[26] == 26 and W.FILLER_LETTER in c.arrays[0][:27 * W.GENE_LEN]            # (the first 27 genes are real: the filler's letter is theirs too)
    assert set(np.unique(c.arrays[0]).tolist()) == set(H.LETTERS.tolist())


def test_above_has_real_genes_and_cells_on_both_sides():
    c = W.case("above")
    real = c.real
    assert (real < B).sum() >= 27 + W.LEAD and (real >= B).sum() > 900
    assert c.first_id[1] == B - W.LEAD and c.first_id[2] > B
    for g in (1, 2):
        col, row = c.want[g]["column"], c.want[g]["row"]
        assert (col < B).any() and (col >= B).mean() > 0.98, g
    assert (c.want[1]["row"] < B).any() and (c.want[1]["row"] >= B).any()                 # genome 1's rows straddle the limit
    assert (c.want[2]["row"] >= B).all()


@pytest.mark.parametrize("name", ["at", "below"])
def test_the_shifted_sets_end_on_a_real_gene_with_cells(name):
    c = W.case(name)
    last = c.n - 1
    assert c.family[last] == W.BIG and (c.want[2]["row"] == last).sum() == 2 * W.N_BIG    # its row: every other member of big
    assert (c.want[1]["column"] == last).sum() == W.N_BIG                                  # ... and it is a column of genome 1's rows


def test_a_truncated_id_cannot_give_the_right_block():
    """small family j: genes j (genome 0), B + j (genome 1) and one of genome 2.  Row j holds column B + j and not j; row B + j holds
    column j and not B + j: whichever way 22 bits of an id are kept, one of the two rows is wrong"""
    c = W.case("above")
    for j in range(W.SMALL):
        ids = c.small_ids(j)
        assert ids.tolist()[:2] == [j, B + j] and len(ids) == 3 and ids[2] > B
        r0 = c.want[0]["column"][c.want[0]["row"] == j]
        r1 = c.want[1]["column"][c.want[1]["row"] == B + j]
        assert sorted(r0.tolist()) == [B + j, int(ids[2])], j
        assert sorted(r1.tolist()) == [j, int(ids[2])], j
        r2 = c.want[2]["column"][c.want[2]["row"] == ids[2]]
        assert sorted(r2.tolist()) == [j, B + j], j                                       # both in one row: neither may become the other


@pytest.mark.parametrize("name", W.SIZES)
def test_rows_for_every_branch_of_k_order(name):
    c = W.case(name)
    for g in (1, 2):
        cells = W.cells_per_row(c.want[g])
        assert ((cells >= 2) & (cells <= W.ORDER_SUB_W)).sum() >= W.SMALL, (name, g)                             # sub-wave rows
        assert ((cells > W.ORDER_SUB_W) & (cells <= W.ORDER_WAVE_CELLS)).sum() >= W.N_WAVE, (name, g)            # a wave's rows
        assert ((cells > W.ORDER_WAVE_CELLS) & (cells <= W.ORDER_ONE_WORD_CELLS)).sum() >= W.N_MID, (name, g)    # order_wide_row, 257-512
        assert (cells > W.ORDER_ONE_WORD_CELLS).sum() >= W.N_BIG and cells.max() == 2 * W.N_BIG, (name, g)       # its general network


def test_the_bounds_are_the_kernels():
    import re
    from pathlib import Path
    src = (Path(__file__).resolve().parents[1] / "pandelos_amd" / "csrc" / "pdl_join.hip").read_text()
    assert re.search(r"ORDER_SUB_W = (\d+);", src).group(1) == str(W.ORDER_SUB_W)
    assert re.search(r"ORDER_CPL = (\d+);", src).group(1) == str(W.ORDER_WAVE_CELLS // 64)
    assert f"a.pack_ok && cnt <= {W.ORDER_ONE_WORD_CELLS}" in src


@pytest.mark.parametrize("name", ["above", "lift+"])
def test_groups_and_costs_straddle_the_limit(name):
    c = W.case(name)
    r, gid, start, size = H.rank_groups(c.dictionary)
    seq = r["seq"].astype(np.int64)
    lo = np.minimum.reduceat(seq, start)
    hi = np.maximum.reduceat(seq, start)
    assert ((size >= 2) & (lo < B) & (hi >= B)).sum() > 100                               # groups with members on both sides
    assert (c.total_visited[:B] > 0).any() and (c.total_visited[B:] > 0).any()
    assert (c.kseq[:B] > 0).any() and (c.kseq[B:] > 0).any()
    assert all(x > 0 for x in c.genome_cost) and sum(c.genome_cost) == c.total_cost


def test_the_appended_genome_lifts_the_base_over_the_limit():
    base, union = W.case("lift"), W.case("lift+")
    rq, oq, fq = W.lift_query()
    assert base.genomes == 2 and base.n == B - W.LIFT_UNDER < B and len(fq) == 40
    assert union.genomes == 3 and union.n == base.n + len(fq) >= B
    assert np.array_equal(union.arrays[0][:len(base.arrays[0])], base.arrays[0]) and np.array_equal(union.arrays[1][:base.n + 1], base.arrays[1])
    assert ((union.real >= B).sum(), (union.real < B).sum()) == (len(fq) - W.LIFT_UNDER, 27 + W.REAL_1 + W.LIFT_UNDER)
    for g in (0, 1):                                     # the new genome changes both old blocks: new columns, and at or above B
        old, new = base.want[g], union.want[g]
        assert new["scoresCount"] > old["scoresCount"] and (new["column"] >= B).any() and not (old["column"] >= B).any(), g
        assert new["max_genome_score"].shape[1] == 3 and old["max_genome_score"].shape[1] == 2
        assert union.genome_cost[g] > base.genome_cost[g]
    assert (union.want[2]["row"] < B).any() and (union.want[2]["row"] >= B).any()         # the appended genome's rows straddle the limit


def test_the_hub_query_row_must_leave_the_lds_table():
    import re
    from pathlib import Path
    src = (Path(__file__).resolve().parents[1] / "pandelos_amd" / "csrc" / "pdl_query.h").read_text()
    qj_t, bits = int(re.search(r"QJ_T = (\d+)", src).group(1)), int(re.search(r"QJ_HT_BITS = (\d+)", src).group(1))
    assert W.QUERY_MUST_LEAVE == (1 << bits) - 2 * qj_t + qj_t               # QJ_LIMIT + QJ_T
    h = W.hub()
    base_n = len(h["base"][2])
    assert base_n == B + W.HUBS and h["n"] == base_n + 3
    cols = h["partners"]
    assert len(cols) >= W.HUBS > W.QUERY_MUST_LEAVE and (cols >= B).sum() >= W.HUBS and cols.max() < base_n      # every hub, and no other query gene
    w = h["want"]
    row0 = w["column"][w["row"] == base_n]
    assert B + 17 in row0.tolist() and (row0 >= B).all()                    # the row has cells: the hub it was copied from among them
    assert (w["row"] == base_n + 1).any() and (w["column"][w["row"] == base_n + 1] < B).all()      # the second gene's cells: small family 3, below B
