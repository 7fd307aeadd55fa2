"""The sets of tests/test_gpu_saturated_counts.py have the properties they are built for — checked here without a GPU, from the
CPU oracle's dictionary and cells alone.

A packed range carries min(the row's own count of the k-mer, 1023) in ten bits (gt_pack_range, pdl_groups.h); at 1023 every reader
takes the count from the record in front of the range.  For the first record of a rank-group (the smallest gene id) that word is the
one that carried the head bit, and in the upper-range build nobody else reads it.  So the sets must hold counts just below, at and
above 1023, in group heads as well, in rows every join tier can take."""
import numpy as np
import pytest

from tests import helpers as H

SETS = ["sat:3:1", "sat:3:2", "sat:4:1", "sat:4:2"]
PT_RB, PT_ROWS, PT_HEAVY_CAP = 960, 4, 64                # pdl_join_part.h: ranges per cycle, rows per cycle, listed heavy lookups per cycle
TINY_TIER2_COLUMNS = 384                                 # a row of more columns leaves the tiny tier-2 table for the HBM kernel


def _rows(case):
    """-> (records in group order, group id, group start, group size, postings above each record, ranges per gene, heavy lookups per
    gene).  A lookup is heavy as k_join_part judges it: the row's own count of the k-mer is >= 2, or the posting's is."""
    r, gid, start, size = H.rank_groups(case.dictionary)
    n = case.gs.genes
    above = size[gid] - 1 - (np.arange(len(r)) - start[gid])
    ranges = np.bincount(r["seq"], weights=above > 0, minlength=n).astype(np.int64)
    repeated = np.r_[0, np.cumsum(r["count"] >= 2)]
    repeated_above = repeated[start[gid] + size[gid]] - repeated[np.arange(len(r)) + 1]
    heavy = np.bincount(r["seq"], weights=np.where(r["count"] >= 2, above, repeated_above), minlength=n).astype(np.int64)
    return r, gid, start, size, above, ranges, heavy


def _emitted(case):
    cells = set()
    for s in case.want:
        cells.update(zip(s["row"].tolist(), s["column"].tolist()))
    return cells


@pytest.mark.parametrize("name", SETS)
def test_the_constructed_set_has_the_property_it_is_named_for(name):
    case = H.saturated_case(name)
    k, gs = case.k, case.gs
    r, gid, start, size, above, ranges, heavy = _rows(case)
    counts = set(r["count"].tolist())
    assert {1022, 1023, 1024} <= counts and max(counts) >= 3000          # below the field's maximum, at it, above, far above
    assert np.all(np.diff(gs.genome_of.astype(np.int64)) >= 0)           # genes listed genome by genome: the join's task order is the gene order
    assert case.kseq.min() > 2 * k                                       # tier 0 can take the set
    assert ranges.max() <= PT_RB                                         # every row fits a cycle of the partition tier
    # the head word: the record with the smallest gene id of a saturated group.  The generator cycles the runs by family + genome, so
    # the families with runs[family % 4] = 1022 open their group below the field's maximum, and at k = 3 a gene of another family that
    # holds the k-mer by chance may come first; what the readers need is heads AT the maximum, just above and far above it — and,
    # as the control, saturated records that are not heads (the word in front of their range never carried the bit).
    sat_groups = np.unique(gid[r["count"] >= 1023])
    assert len(sat_groups) == 20 * int(name.split(":")[2])               # every planted k-mer, nothing else
    head_counts = r["count"][start[sat_groups]]
    assert {1023, 1024} <= set(head_counts.tolist()) and head_counts.max() >= 3000
    assert (head_counts >= 1023).sum() * 2 >= len(sat_groups)            # (most groups: three families in four, less the chance members)
    is_head = np.zeros(len(r), bool)
    is_head[start] = True
    assert ((r["count"] >= 1023) & ~is_head & (above > 0)).sum() >= len(sat_groups)
    assert ((r["count"] >= 1023) & is_head & (above > 0)).sum() == (head_counts >= 1023).sum()      # (every such head has a range: it is read again)
    # heavy lookups: four rows of a cycle share a list of PT_HEAVY_CAP entries.  At k = 4 a row has 16 at most; at k = 3 genes of
    # different families share k-mers by chance (80 genes x 220 k-mers over 8000), a row stays below the list's size by itself.
    assert heavy.max() <= (PT_HEAVY_CAP // PT_ROWS if k >= 4 else PT_HEAVY_CAP - 1), heavy.max()
    # a cell whose two genes hold a shared k-mer more than 1023 times EACH: only there does min(column's count, row's count) depend on
    # the re-read (percs depends on it in every cell of such a row)
    cells, both = _emitted(case), 0
    for g in sat_groups:
        m = r[start[g]:start[g] + size[g]]
        over = m["seq"][m["count"] > 1023].tolist()
        both += sum((a, b) in cells for a in over for b in over if a < b)
    assert both >= 1


def test_the_dense_set_sends_its_rows_to_the_hbm_kernel():
    case = H.saturated_case("dense")
    r, gid, start, size, above, ranges, heavy = _rows(case)
    n = case.gs.genes
    sat_groups = np.unique(gid[r["count"] >= 1023])
    assert len(sat_groups) == 1 and size[sat_groups[0]] == n             # one planted k-mer, in every gene
    g = sat_groups[0]
    m = r[start[g]:start[g] + n]
    assert np.array_equal(m["seq"], np.arange(n))
    assert m["count"][0] == 1023                                         # the head's own count is saturated: its word is read again
    assert {1022, 1023, 1100, 2500} <= set(m["count"].tolist())
    columns = above[start[g]:start[g] + n]                               # gene i's range of it: the n - 1 - i genes above
    assert np.all(columns[:n - TINY_TIER2_COLUMNS - 1] > TINY_TIER2_COLUMNS)
    assert case.kseq.min() > 2 * case.k and len(_emitted(case)) > 100000


@pytest.mark.parametrize("variant", ["head", "middle", "same_gene_twice"])
def test_the_fold_sets_fold_a_saturated_singleton(variant):
    gs, x = H.fold_saturated_set(variant)
    case = H.OracleCase(gs, 3)
    d = case.dictionary
    top = d["rank"].max()
    last = d[d["rank"] == top]
    assert len(last) == 1 and last["seq"][0] == x and last["count"][0] == 3000       # the globally last record: a singleton, 3000 times in gene X
    r, gid, start, size = H.rank_groups(d)
    grp = r[start[-1]:]
    others = grp[grp["rank"] != top]
    assert len(set(others["rank"].tolist())) == 1 and len(others) >= 2                # folded into the motif's group
    assert (x in others["seq"].tolist()) == (variant == "same_gene_twice")
    at = int(np.flatnonzero(grp["rank"] == top)[0])
    assert (at == 0) == (variant == "head") and at < len(grp) - 1                     # head of the group or inside it; postings above it either way
    assert any(x in (a, b) for a, b in _emitted(case))                                # X's cells are observable
