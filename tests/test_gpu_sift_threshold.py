"""Tier 0's sift by the validity threshold ("sift_threshold", k_join_part in pdl_join_part.h): a column goes to the table
only when the cycle's counter of it reached T = clamp(min(tc_min, min pc_min of the cycle's rows), 2, 255).  Every set below is
built for one property of that rule; the property is checked on the CPU first (k-mers counted with numpy, cells taken from
the oracle), then every genome of the GPU result is compared field by field with the oracle, with the rule on and off
("sift_threshold" 1 / 0; off = T forced to 2 on the counters).  The counters are taken where the set's threshold is at least
SIFT_T_MIN (PT_SIFT_T_MIN in pdl_join_part.h); below it the kernel's bitmap form runs, the "seen twice" sift — so the sets of a
low threshold go through the bitmaps with the rule on and through the counters with it off."""
import functools

import numpy as np
import pytest

from tests import helpers as H

K = 5
SIFT_T_MIN = 4
LETTERS = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)


# ---- the device's arithmetic, restated -----------------------------------------------------------------------------------
def _min_numerator(denom: int, k: int = K) -> int:
    """smallest n with n / denom >= 1 / 2k in float32 (min_numerator in pdl_join.hip)"""
    thr, d, n = np.float32(1.0) / np.float32(2.0 * k), np.float32(denom), 0
    while np.float32(n) / d < thr:
        n += 1
    return n


def _sift_t(min_kseq: int, row_kseqs) -> int:
    return max(2, min(255, min(_min_numerator(min_kseq), min(_min_numerator(v) for v in row_kseqs))))


# ---- k-mers on the host --------------------------------------------------------------------------------------------------
def _codes(gene) -> np.ndarray:
    c = np.searchsorted(LETTERS, gene).astype(np.int64)
    n = len(c) - K + 1
    v = np.zeros(n, np.int64)
    for j in range(K):
        v = v * 20 + c[j:j + n]
    return v


def _shared(a, b):
    """-> (light, heavy): k-mers of genes a and b with count 1 on both sides / a count >= 2 on either"""
    ua, ca = np.unique(_codes(a), return_counts=True)
    ub, cb = np.unique(_codes(b), return_counts=True)
    both, ia, ib = np.intersect1d(ua, ub, return_indices=True)
    heavy = (ca[ia] >= 2) | (cb[ib] >= 2)
    return int((~heavy).sum()), int(heavy.sum())


def _upper_rows(genes):
    """per gene: (ranges, lookups) of its row above the diagonal — its k-mers that a later gene holds too, and those genes"""
    code = np.concatenate([np.unique(_codes(g)) for g in genes])
    gene = np.concatenate([np.full(len(np.unique(_codes(g))), i) for i, g in enumerate(genes)])
    o = np.lexsort((gene, code))
    code, gene = code[o], gene[o]
    start = np.flatnonzero(np.r_[True, code[1:] != code[:-1]])
    end = np.repeat(np.r_[start[1:], len(code)], np.diff(np.r_[start, len(code)]))
    after = end - np.arange(len(code)) - 1
    ranges = np.bincount(gene, weights=after > 0, minlength=len(genes)).astype(np.int64)
    lookups = np.bincount(gene, weights=after, minlength=len(genes)).astype(np.int64)
    return ranges, lookups


def _flatten(genes, genome_of):
    off = np.zeros(len(genes) + 1, np.uint64)
    np.cumsum([len(g) for g in genes], out=off[1:])
    return np.concatenate(genes).astype(np.uint8), off, np.asarray(genome_of, np.uint32)


def _rand(rng, n):
    return LETTERS[rng.integers(0, 20, n)]


def _other(letter):
    return LETTERS[(int(np.searchsorted(LETTERS, letter)) + 1) % 20]


# ---- the sets ------------------------------------------------------------------------------------------------------------
def _pair_set(seed, row_len, col_len, n_shared, filler_len, repeat=None):
    """Gene 0 (the row, genome 0) and the last gene (the column, genome 2) share one stretch of n_shared k-mers; eight unrelated
    genes of filler_len residues lie between them.  repeat = (times in the row, times in the column): one more k-mer, planted
    that often on each side."""
    rng = np.random.Generator(np.random.PCG64(seed))
    row, col = _rand(rng, row_len), _rand(rng, col_len)
    w, at = n_shared + K - 1, min(10, (col_len - n_shared - K + 1) // 2)
    col[at:at + w] = row[20:20 + w]
    col[at - 1], col[at + w] = _other(row[19]), _other(row[20 + w])     # (the stretch ends where it ends)
    if repeat:
        motif = _rand(rng, K)
        for t in range(repeat[0]):
            row[row_len - 12 - 9 * t:row_len - 12 - 9 * t + K] = motif
        for t in range(repeat[1]):
            col[col_len - 8 - 9 * t:col_len - 8 - 9 * t + K] = motif
    genes = [row] + [_rand(rng, filler_len) for _ in range(8)] + [col]
    return genes, [0, 0, 0, 0, 1, 1, 1, 1, 2, 2]


def _build(name):
    """-> (genes, genome_of)"""
    kind, _, arg = name.partition(":")
    if kind == "tc_binds":        # the column is by far the shortest gene: T = tc_min = what the COLUMN needs (100 k-mers: 10); the row needs 40
        return _pair_set(11, 400, 104, 10 + int(arg), 300)
    if kind == "pc_binds":        # only long genes, the row the shortest: T = its pc_min (200 k-mers: 20); the column needs 60.  (The row being the
                                  # set's shortest gene, tc_min is 20 as well: no row's pc_min can be BELOW tc_min, a row has min_kseq k-mers at least.
                                  # What differs from tc_binds is the side that makes the cell valid: perc here, tr_perc there.)
        return _pair_set(12, 204, 604, 20 + int(arg), 500)
    if kind == "floor":           # the shortest gene has 2k + 1 k-mers: tc_min = 2, the "seen twice" rule; it shares 2 k-mers with the row
        return _pair_set(13, 300, 2 * K + 1 + K - 1, 2, 200)
    if kind == "low":             # the set's threshold just below / at SIFT_T_MIN (the column has 30 / 40 k-mers: 3 / 4): bitmaps / counters; T shared k-mers
        t = int(arg)
        return _pair_set(18 + t, 300, 10 * t + K - 1, t, 200)
    if kind == "heavy":           # 7 light k-mers beside one that the row holds twice and the column three times: tc = 7 + 3 = 10 of 100
        return _pair_set(14, 400, 104, 7, 300, repeat=(2, 3))
    if kind == "cap":             # genes of 3000+ k-mers only: pc_min >= 300, T = 255; the row shares 400 / 280 / 200 k-mers with three columns
        rng = np.random.Generator(np.random.PCG64(15))
        row = _rand(rng, 3300)
        genes, at = [row], 50
        for n in (400, 280, 200):
            col = _rand(rng, 3100 + n)
            col[100:100 + n + K - 1] = row[at:at + n + K - 1]
            col[99], col[100 + n + K - 1] = _other(row[at - 1]), _other(row[at + n + K - 1])
            at += n + 60
            genes.append(col)
        fill = [_rand(rng, 3200) for _ in range(2)]
        return [genes[0], genes[1], fill[0], genes[2], fill[1], genes[3]], [0, 1, 1, 2, 2, 3]      # (the columns: genes 1, 3, 5)
    if kind == "shared":          # 6000+ short genes: more columns than counters; genes 0-3 are four copies of one gene (one cycle) that meet the same columns
        from pandelos_amd.synth import make_gene_set
        gs = make_gene_set(genomes=8, genes_per_genome=1000, mean_len=80, sub_rate=0.05, seed=16)
        off = gs.offsets.astype(np.int64)
        long_enough = np.flatnonzero(np.diff(off) >= 64)         # (60 k-mers at least: the threshold is 6, not the floor)
        genes = [gs.residues[off[i]:off[i + 1]] for i in long_enough]
        genome_of = gs.genome_of[long_enough]
        rng = np.random.Generator(np.random.PCG64(17))
        assert (gs.family_of[long_enough] == gs.family_of[long_enough][40]).sum() >= 5      # (the copies' family is in most genomes)
        copies = []
        for _ in range(4):
            c = genes[40].copy()
            c[rng.integers(0, len(c), 2)] = _rand(rng, 2)
            copies.append(c)
        return copies + genes, [0, 0, 0, 0] + [int(g) for g in genome_of]
    if kind == "both_forms":      # ~70 close homologs per gene: rows of 4-8 k lookups take the 512-thread form
        from pandelos_amd.synth import make_gene_set
        gs = make_gene_set(genomes=70, genes_per_genome=60, mean_len=250, sub_rate=0.03, seed=7703)
        off = gs.offsets.astype(np.int64)
        return [gs.residues[off[i]:off[i + 1]] for i in range(gs.genes)], [int(g) for g in gs.genome_of]
    raise KeyError(name)


CASES = ["low:3", "low:4", "tc_binds:-1", "tc_binds:0", "tc_binds:1", "pc_binds:-1", "pc_binds:0", "pc_binds:1", "floor", "heavy", "shared", "both_forms", "cap"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (genes, (residues, offsets, genome_of), the oracle's Scores of every genome); computed once, never changed"""
    from oracle import binding as ob
    genes, genome_of = _build(name)
    flat = _flatten(genes, genome_of)
    ora = ob.Oracle(*flat, K)
    want = [ora.scores(g) for g in range(ora.genomes)]
    assert np.array_equal(ora.kseq_lengths(), [len(g) - K + 1 for g in genes])
    ora.close()
    return genes, flat, want


def _cell(want, genome_of, r, c):
    """the oracle's cell (row gene r, column gene c) as (score, perc, tr_perc), or None when it was not emitted"""
    s = want[genome_of[r]]
    hit = np.flatnonzero((s["row"] == r) & (s["column"] == c))
    assert len(hit) <= 1
    return (float(s["scores"][hit[0]]), float(s["percs"][hit[0]]), float(s["tr_percs"][hit[0]])) if len(hit) else None


def _check_property(name):
    """what the set is named for, from the host's k-mer counts and the oracle's cells alone"""
    genes, (res, off, gen), want = _case(name)
    kseq = [len(g) - K + 1 for g in genes]
    assert min(kseq) > 2 * K                                      # (tier 0 can be selected)
    assert np.all(np.diff(gen.astype(np.int64)) >= 0)             # genes listed genome by genome: the join's task order (genomes in order, a genome's
                                                                  # genes in order) is the gene order, rows are drawn eight at a time from gene 0 on, and
                                                                  # genes 0..3 are the first cycle's candidates
    ranges, lookups = _upper_rows(genes)
    kind, _, arg = name.partition(":")
    last = len(genes) - 1
    if kind in ("tc_binds", "pc_binds"):
        d = int(arg)
        t = _sift_t(min(kseq), kseq[0:4])                        # (gene 0's cycle: the first rows of its draw)
        light, heavy = _shared(genes[0], genes[last])
        assert (light, heavy) == (t + d, 0), (light, heavy, t)
        pc_min, tc_min = _min_numerator(kseq[0]), _min_numerator(min(kseq))
        if kind == "tc_binds":
            assert kseq[last] == min(kseq) and t == tc_min == 10 and pc_min == 40
        else:
            assert kseq[0] == min(kseq) and t == pc_min == 20 and _min_numerator(kseq[last]) == 60
        cell = _cell(want, gen, 0, last)
        assert (cell is not None) == (d >= 0), (name, cell)        # emitted at T and T + 1, absent at T - 1
    elif kind == "low":
        t = int(arg)
        assert t == _sift_t(min(kseq), kseq[0:4]) == _min_numerator(kseq[last]) and kseq[last] == min(kseq) and (t >= SIFT_T_MIN) == (t == 4)
        assert _shared(genes[0], genes[last]) == (t, 0) and _cell(want, gen, 0, last) is not None
    elif kind == "floor":
        assert kseq[last] == 2 * K + 1 == min(kseq) and _min_numerator(min(kseq)) == 2 and _sift_t(min(kseq), kseq[0:4]) == 2
        assert _shared(genes[0], genes[last]) == (2, 0) and _cell(want, gen, 0, last) is not None
    elif kind == "heavy":
        t = _sift_t(min(kseq), kseq[0:4])
        assert _shared(genes[0], genes[last]) == (7, 1) and t == 10 and 7 < t
        cell = _cell(want, gen, 0, last)                          # tc = 7 + 3 of 100 k-mers: valid only with the light ones counted
        assert cell is not None and np.float32(cell[2]) == np.float32(10) / np.float32(kseq[last])
        assert np.float32(cell[1]) == np.float32(7 + 2) / np.float32(kseq[0])
    elif kind == "cap":
        assert all(_min_numerator(v) > 255 for v in kseq) and _sift_t(min(kseq), kseq) == 255
        assert all(r <= 960 and lk <= 4096 for r, lk in zip(ranges, lookups))          # (every row fits a cycle of the first form)
        shared = [_shared(genes[0], genes[c])[0] for c in (1, 3, 5)]
        assert shared[0] >= 340 and 255 <= shared[1] < 300 and 150 <= shared[2] < 255, shared      # (all three columns: enough for the row? enough for the sift?)
        assert [_cell(want, gen, 0, c) is not None for c in (1, 3, 5)] == [True, False, False]
    elif kind == "shared":
        assert len(genes) > 4096 + 1500
        assert ranges[0:4].sum() <= 960 and lookups[0:4].sum() <= 4096                 # genes 0-3 are one cycle ...
        cols = [set(np.flatnonzero([_shared(genes[r], genes[c])[0] >= 10 for c in range(4, 400)]) + 4) for r in range(4)]
        assert len(set.intersection(*cols)) >= 1                                         # ... and meet one column at least, all four
        assert _sift_t(min(kseq), kseq[0:4]) > 2
    elif kind == "both_forms":
        assert ((lookups > 4096) & (lookups <= 8192) & (ranges <= 960)).sum() >= 100   # rows of the second form
        assert (lookups <= 4096).sum() >= 100                                            # and of the first
        assert _sift_t(min(kseq), [min(kseq)]) > 2


@pytest.mark.parametrize("name", CASES)
def test_the_constructed_set_has_the_property_it_is_named_for(name):
    _check_property(name)


@pytest.mark.gpu
@pytest.mark.parametrize("sift", [1, 0])
@pytest.mark.parametrize("name", CASES)
def test_tier0_matches_the_oracle_with_the_sift_by_threshold_on_and_off(name, sift):
    from pandelos_amd.pangene_native import PangeneNative
    _check_property(name)
    genes, (res, off, gen), want = _case(name)
    nat = PangeneNative.open()
    nat.set_option("join_tier0", 1)
    nat.set_option("sift_threshold", sift)
    nat.preprocess(K, res, off, gen)
    got = [nat.generate_scores_part(g).as_dict() for g in range(len(want))]
    tm = nat.timings()
    nat.close()
    for g in range(len(want)):
        H.assert_scores_equal(got[g], want[g], f"{name} sift_threshold={sift} genome {g}")
    assert tm["aside_reloads"] == 0 and tm["tier1_rows"] < tm["scored_rows"]           # (tier 0 took rows)
    if name != "both_forms":
        assert tm["tier1_rows"] == 0                                                     # every row stayed in tier 0
    kind, _, arg = name.partition(":")
    if kind in ("tc_binds", "pc_binds"):                                                 # the pair itself, in the GPU's own cells
        s, last = got[0], len(genes) - 1
        assert bool(np.any((s["row"] == 0) & (s["column"] == last))) == (int(arg) >= 0)


@pytest.mark.gpu
def test_sift_threshold_takes_0_or_1_only():
    from pandelos_amd._lib import PdlError
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.open()
    for bad in (-1, 2, 255):
        with pytest.raises(PdlError):
            nat.set_option("sift_threshold", bad)
    nat.set_option("sift_threshold", 0)
    nat.set_option("sift_threshold", 1)
    nat.close()
