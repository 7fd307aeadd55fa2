"""The sets of tests/test_gpu_join_edges.py are what they claim — checked here without a GPU, against the CPU oracle's dictionary
(helpers.rank_groups: the groups as the reference's scan forms them), its cells and a plain numpy k-mer count.

For every set the GPU file uses:
  a  each planted row's ranges, in rank order, have exactly the planned lengths, hold exactly the planned columns, its heavy lookups
     are exactly the planned ones, and the oracle's block gives it the cell count the fillers were sized for
  b  neither the record the reference folds nor the group in front of it touches a planted row
  c  every unplanted gene shares k-mers with no more genes than the set declares: 64, or — where the planted row has ranges longer
     than that, whose columns cannot help sharing the row's word with each other — a bound the set works out from its incidence,
     which the GPU file holds against the table's LIMIT before it asserts that only the planted row leaves a table
  d  unless the case plants a short gene, min kseq > 2k
  e  the table of limits is consistent with itself and with the figures DESIGN.md prints"""
import numpy as np
import pytest

from tests import helpers as H
from tests import join_edge_sets as J

NAMES = J.all_names()


def _kmer_counts(gs, gene, k):
    """{k-mer bytes: count} of one gene, plainly"""
    off = gs.offsets.astype(np.int64)
    s = gs.residues[off[gene]:off[gene + 1]].tobytes()
    out = {}
    for i in range(len(s) - k + 1):
        out[s[i:i + k]] = out.get(s[i:i + k], 0) + 1
    return out


def test_the_table_of_limits_is_consistent():
    assert set(J.FORMS) == set(J.LIMITS)
    for name, f in J.FORMS.items():
        limit, touch_cap, rb = J.LIMITS[name]
        assert f.limit == f.ht - f.threads - f.ht // 8 == limit, name
        assert f.touch_cap == f.limit + f.threads == touch_cap < f.ht, name
        assert f.rb == (2 * f.threads if f.filtered else f.threads) == rb, name
        assert f.threads % 64 == 0 and f.chunks_per_step in (4, 8)
    assert J.PT_LMAX[256] == 16 * 256 and J.PT_LMAX[512] == 2 * J.PT_LMAX[256] and J.PT_RB % 64 == 0 and J.PT_RB <= 1022
    assert J.PT_PART_KEYS == {1: 768, 2: 384, 3: 192, 4: 192} and all(J.PT_PART[n] * min(n, 4) <= J.PT_HT for n in J.PT_PART)
    assert J.defer_cap(100) == 164 and J.defer_cap(20000) == 8192 and J.defer_cap(20000, 5000) == 20000


def test_the_names_are_distinct_and_cover_every_section():
    assert len(set(NAMES)) == len(NAMES)
    assert {n[0] for n in NAMES} == {"A", "B", "C", "D", "E", "FA", "FD"}


def test_a_plain_kmer_count_agrees_with_the_incidence():
    """the builder's text against its own plan, without the oracle: the planted row holds each of its words `own` times, the word's
    other holders are the planned columns with the planned counts, and no other window of the row is in any other gene"""
    name = ("D", "tiny2", "mix", 1)
    pl = J.planted(name)
    gs, row, g = pl.gs, pl.rows[0], pl.row_genes[0]
    mine = _kmer_counts(gs, g, J.K)
    holders = {}
    for other in range(gs.genes):
        if other != g:
            for w, n in _kmer_counts(gs, other, J.K).items():
                if w in mine:
                    holders.setdefault(w, {})[other] = n
    shared = sorted(holders)                             # bytes order = rank order
    assert len(shared) == row.nr
    for i, w in enumerate(shared):
        assert mine[w] == row.own[i]
        assert holders[w] == {int(pl.column_gene[c]): int(n) for c, n in zip(row.cols[i], row.ccnt[i])}


@pytest.mark.parametrize("name", NAMES, ids=J.ident)
def test_the_set_is_what_it_claims(name):
    pl, case = J.planted(name), J.case(name)
    d = J.describe(case, pl)
    planted_genes = set(pl.row_genes)
    cells = np.concatenate([w["row"] for w in case.want])
    for row, g, got in zip(pl.rows, pl.row_genes, d["rows"]):
        # a: the ranges (a shard keeps whole groups; describe() leaves the row itself out either way)
        assert np.array_equal(got["lens"], row.lens), f"{name}: range lengths of row {g}"
        for i in range(row.nr):
            assert np.array_equal(np.sort(got["cols"][i]), np.sort(pl.column_gene[row.cols[i]])), f"{name}: columns of range {i} of row {g}"
        assert np.array_equal(got["own"], row.own)
        if not pl.middle:                                # (below the row the postings keep gene order, not the plan's)
            assert np.array_equal(got["heavy"], row.heavy), f"{name}: heavy lookups of row {g}"
        assert got["heavy"].sum() == row.heavy.sum()
        assert len(np.unique(np.concatenate(got["cols"]))) == len(row.columns)
        # ... and the oracle emits the row's cell of every column sighted often enough for its filler (twice; four times with long
        # fillers), in the row's block when the column lies above it
        sight = np.bincount(np.concatenate(row.cols), weights=np.concatenate(row.ccnt))
        want_cells = int((sight >= 2).sum())
        have = int((cells == g).sum())
        assert have == want_cells, f"{name}: row {g} has {have} cells, {want_cells} planned"
    # b: the fold
    assert not (planted_genes & set(d["fold"])), f"{name}: the fold touches a planted row"
    # c: the unplanted genes
    others = np.setdiff1d(np.arange(case.gs.genes), pl.row_genes)
    assert d["partners"][others].max() <= pl.unplanted_partners, f"{name}: an unplanted gene has {d['partners'][others].max()} partners"
    # d: the shortest gene
    if pl.short_gene:
        assert case.kseq.min() == pl.short_gene
    else:
        assert case.kseq.min() > 2 * J.K


@pytest.mark.parametrize("name", [n for n in J.names_e() if n[2] > 1 and n[1] != "columns"], ids=J.ident)
def test_the_rows_of_a_packed_tier_0_cycle_fit_their_parts_of_the_table(name):
    """A cycle whose part of the table overflows is thrown away and its rows are run again one by one: the packed cycle would be
    walked and never compared.  So outside the "columns" sets, which are about that limit, every planted row of a multi-row set
    keeps its columns (= its keys at most) within the keys its part takes, and the rows fit one cycle's ranges but for the last."""
    pl = J.planted(name)
    rows = name[2]
    for r in pl.rows:
        assert len(r.columns) <= J.PT_PART_KEYS[rows], f"{name}: {len(r.columns)} columns in a part of {J.PT_PART_KEYS[rows]} keys"
    assert sum(r.nr for r in pl.rows[:-1]) < J.PT_RB and sum(r.lookups for r in pl.rows[:-1]) < J.PT_LMAX[256]


@pytest.mark.parametrize("fname", J.B_FORMS)
def test_the_exactly_full_row_fills_a_wave_s_part(fname):
    """the prediction the sweep of section B stands on, restated from the incidence: wave 0's segment holds the singles and both
    sightings of its own columns and nothing else, and the eight paddings put its count inside the parts they make"""
    form = J.FORMS[fname]
    row, columns, lo, hi = J.exactly_full(form)
    chunks = -(-row.lookups // 64)
    seg = -(-chunks // form.waves) * 64                  # pdl_join.hip:349-350
    flat = np.concatenate(row.cols)
    sight = np.bincount(flat)
    for w in range(form.waves):
        inside = np.unique(flat[w * seg:(w + 1) * seg])
        assert np.isin(flat[:w * seg], inside).sum() == 0 and np.isin(flat[(w + 1) * seg:], inside).sum() == 0     # no column in two segments
    first = np.unique(flat[:seg])
    assert len(flat[:seg]) == seg == (sight[first] == 1).sum() + 2 * (sight[first] == 2).sum()
    assert lo <= hi <= len(first) and hi - lo <= 8       # (hi: the distinct bits of wave 0's columns; lo: less those another wave's column shares)
    assert (sight == 2).sum() == form.limit - 1 and (sight == 1).sum() == (sight[first] == 1).sum()
    bits = J.bitmap_bit(form, 1 + np.arange(len(sight)))
    singles = np.flatnonzero(sight == 1)
    assert len(set(bits[singles].tolist())) == len(singles) and not set(bits[singles].tolist()) & set(bits[sight == 2].tolist())
    parts = [J.planted(("B", fname, "full", i)).note["part"] for i in range(8)]
    assert parts == list(range(hi - 4, hi + 4)) and parts[0] < lo
    for w in range(1, form.waves):                       # the other waves file fewer
        assert len(np.unique(flat[w * seg:(w + 1) * seg])) < parts[0]
