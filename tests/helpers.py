"""Shared test helpers: golden fixture access and bit-exact Scores comparison."""
from __future__ import annotations

import hashlib
import json
import tempfile
from pathlib import Path

import numpy as np

from pandelos_amd.pangene_idata import PangeneIData
from pandelos_amd.synth import make_gene_set

GOLDEN = Path(__file__).resolve().parent / "golden"
FIELDS = ("scores", "percs", "tr_percs", "row", "column", "first_seq_genome", "second_seq_genome",
          "max_genome_score", "max_genome_score_col", "scoresMaxMappings")
SMALL_CASES = sorted(p.stem for p in GOLDEN.glob("*.npz"))
DIGESTS = json.loads((GOLDEN / "digests.json").read_text())


def raw(a):
    """float32 arrays are compared as bit patterns; everything else as is."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def load_small(name):
    """-> (residues, offsets, genome_of, k, fixture dict) for one tests/golden/<name>.npz"""
    fx = dict(np.load(GOLDEN / f"{name}.npz"))
    with tempfile.NamedTemporaryFile(suffix=".faa") as f:
        f.write(fx["faa"].tobytes())
        f.flush()
        data = PangeneIData.read_from_file(f.name)
    res, off, gen = data.flatten()
    return res, off, gen, int(fx["k"]), fx


def load_large(name):
    d = DIGESTS[name]
    gs = make_gene_set(**d["shape"])
    return gs.residues, gs.offsets, gs.genome_of, d["k"], d


def assert_scores_equal_fixture(get_scores, fx, genomes, label=""):
    """get_scores(g) -> dict of numpy arrays with the Scores field names."""
    for g in range(genomes):
        got = get_scores(g)
        for f in FIELDS:
            want = fx[f"g{g}_{f}"]
            have = raw(got[f])
            assert have.shape == want.shape, f"{label} genome {g} field {f}: shape {have.shape} != {want.shape}"
            assert np.array_equal(have, want), f"{label} genome {g} field {f} differs"


def assert_scores_match_digest(get_scores, d, label=""):
    for g in range(d["genomes"]):
        got = get_scores(g)
        assert int(got["scoresCount"]) == d["scoresCount"][g], f"{label} genome {g} scoresCount"
        for f in FIELDS:
            h = hashlib.sha256(raw(got[f]).tobytes()).hexdigest()
            assert h == d["sha256"][g][f], f"{label} genome {g} field {f} digest differs"


def assert_scores_equal(a: dict, b: dict, label=""):
    for f in FIELDS:
        x, y = raw(a[f]), raw(b[f])
        assert x.shape == y.shape, f"{label} field {f}: shape {x.shape} != {y.shape}"
        if not np.array_equal(x, y):
            bad = np.nonzero(x.reshape(-1) != y.reshape(-1))[0]
            raise AssertionError(f"{label} field {f}: {len(bad)} mismatches, first at {bad[:5]}")


# ---- genome-pair sampling of a set too large for the reference (configs[4]) ------------------------------------------
# A cell's three values depend on the two genes alone (their k-mer multisets under the same k and the same alphabet ranks):
# the cells of rows of genome A against columns of genome B are the same whether the dictionary was built from all 512
# genomes or from a handful of them — except around the reference's fold of the globally LAST record into the preceding
# rank-group (library.cpp:300-306), which touches only cells of the gene that holds that record.  So the reference run on a
# few genomes pins those genome pairs of the full run, once the genes holding the largest-rank k-mer (of the subset and of
# the full set) are left out on both sides.
LETTERS = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)


def genes_holding_the_largest_kmer(residues, offsets, k, gene_ids=None):
    """Global ids of the genes that contain an occurrence of the largest-rank k-mer (ranks = base-20 numbers over LETTERS in
    ascending letter order, library.cpp:96-100,134-150) among `gene_ids` (default: all genes).  Chunked: the full
    512-genome set is 0.9 G residues."""
    code = np.full(256, 255, np.uint8)
    code[LETTERS] = np.arange(20, dtype=np.uint8)
    off = np.asarray(offsets, dtype=np.int64)
    ids = np.arange(len(off) - 1, dtype=np.int64) if gene_ids is None else np.asarray(gene_ids, dtype=np.int64)
    best, holders = -1, []
    step = 4096
    for i0 in range(0, len(ids), step):
        part = ids[i0:i0 + step]
        contiguous = len(part) and part[-1] - part[0] + 1 == len(part)
        for lo, hi, genes in ([(int(off[part[0]]), int(off[part[-1] + 1]), part)] if contiguous
                              else [(int(off[g]), int(off[g + 1]), np.array([g])) for g in part]):
            c = code[residues[lo:hi]].astype(np.int64)
            assert c.max(initial=0) < 20
            n = len(c) - k + 1
            if n <= 0:
                continue
            v = np.zeros(n, np.int64)
            for j in range(k):
                v = v * 20 + c[j:j + n]
            # k-mers must not straddle genes: position p (chunk-local) belongs to gene `gi`, valid iff p + k <= end of that gene
            ends = off[genes + 1] - lo
            gi = np.searchsorted(ends, np.arange(n), side="right")
            v[np.arange(n) + k > ends[np.minimum(gi, len(ends) - 1)]] = -1
            m = int(v.max())
            if m > best:
                best, holders = m, []
            if m == best and m >= 0:
                holders.extend(int(genes[x]) for x in np.unique(gi[v == m]))
    return sorted(set(holders))


def pair_cells_digest(block, first_gene_a, first_gene_b, genome_b, excluded_a=(), excluded_b=()):
    """SHA-256 (and count) of the cells of one Scores block (rows of genome A) whose column lies in genome B, as sorted
    (row - first gene of A, column - first gene of B, score bits, perc bits, tr bits); cells of excluded local genes left out."""
    sel = np.asarray(block["second_seq_genome"]) == genome_b
    r = np.asarray(block["row"])[sel].astype(np.int64) - first_gene_a
    c = np.asarray(block["column"])[sel].astype(np.int64) - first_gene_b
    keep = ~np.isin(r, np.asarray(list(excluded_a), dtype=np.int64)) & ~np.isin(c, np.asarray(list(excluded_b), dtype=np.int64))
    r, c = r[keep], c[keep]
    o = np.lexsort((c, r))
    h = hashlib.sha256()
    h.update(r[o].astype("<i4").tobytes()); h.update(c[o].astype("<i4").tobytes())
    for f in ("scores", "percs", "tr_percs"):
        h.update(raw(np.asarray(block[f])[sel][keep][o]).astype("<u4").tobytes())
    return h.hexdigest(), int(len(r))


def wrapped_rank_set(letters: int, seed: int, genomes: int = 4, per_genome: int = 12, length: int = 70):
    """A small set over `letters` distinct ASCII letters — for k so large that B^k passes 2^64 while rank_init's overflow test
    (library.cpp:104-111: wrapped products, one multiplication ahead) does not notice, e.g. 22 letters at k = 15, 24 at k = 14:
    the ranks are then the polynomial mod 2^64 and fill all 64 bits although rank_init sees fewer.  -> pandelos_amd.synth.GeneSet"""
    from pandelos_amd.synth import GeneSet
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz", dtype=np.uint8)[:letters]
    fams = [alpha[rng.integers(0, letters, int(rng.integers(length // 2, length * 2)))] for _ in range(per_genome)]
    genes, gen, fam_of = [], [], []
    for g in range(genomes):
        for f, base in enumerate(fams):
            if rng.random() < 0.15:
                continue
            s = base.copy()
            m = rng.random(len(s)) < 0.05
            s[m] = alpha[rng.integers(0, letters, int(m.sum()))]
            genes.append(s); gen.append(g); fam_of.append(f)
    genes[0][:letters] = alpha                       # every letter occurs
    offsets = np.zeros(len(genes) + 1, np.uint64)
    np.cumsum([len(x) for x in genes], out=offsets[1:])
    return GeneSet(np.concatenate(genes).astype(np.uint8), offsets, np.asarray(gen, np.uint32), np.asarray(fam_of, np.int64))


# ---- k-mers that occur 1023 times or more inside one gene ---------------------------------------------------------------------
# The single-GPU build packs a row's range into 8 bytes with the row's own count of the k-mer in a 10-bit field (gt_pack_range in
# pdl_groups.h: min(count, 1023)); a reader that finds 1023 there takes the true count from the record in front of the range.  The
# sets below plant such k-mers: a stretch of `runs[i]` repeats of a unit of `period` letters has runs[i] occurrences of each of the
# `period` k-mers that lie inside it.
SATURATED_RUNS = (1022, 1023, 1024, 3000)                # below the field's maximum, the maximum, above it, far above it


def _as_gene_set(genes, genome_of, family_of):
    from pandelos_amd.synth import GeneSet
    offsets = np.zeros(len(genes) + 1, np.uint64)
    np.cumsum([len(x) for x in genes], out=offsets[1:])
    return GeneSet(np.concatenate(genes).astype(np.uint8), offsets, np.asarray(genome_of, np.uint32), np.asarray(family_of, np.int64))


as_gene_set = _as_gene_set


SIFT_T_MIN = 4                                           # PT_SIFT_T_MIN in pdl_join_part.h: below it the partition tier runs its bitmap form


def min_numerator(denom: int, k: int) -> int:
    """smallest n with n / denom >= 1 / 2k in float32 (min_numerator in pdl_join.hip)"""
    thr, d, n = np.float32(1.0) / np.float32(2.0 * k), np.float32(denom), 0
    while np.float32(n) / d < thr:
        n += 1
    return n


def sift_form(kseq_min: int, k: int, sift_threshold: int = 1) -> str:
    """the form of the partition tier the host launches for a set (score_plan, pdl_join.hip:1739-1741): "counters" when the set's
    threshold clamp(tc_min, 2, 255) reaches SIFT_T_MIN or option "sift_threshold" is 0, and "bitmaps" otherwise"""
    return "counters" if sift_threshold == 0 or max(2, min(255, min_numerator(kseq_min, k))) >= SIFT_T_MIN else "bitmaps"


def stretch(unit, repeats: int, k: int) -> np.ndarray:
    """`unit` repeated until every k-mer inside the stretch occurs `repeats` times: repeats * len(unit) + k - 1 residues"""
    unit = np.asarray(unit, np.uint8)
    n = repeats * len(unit) + k - 1
    return np.tile(unit, n // len(unit) + 1)[:n]


def saturated_count_set(k: int, period: int = 1, fams: int = 20, genomes: int = 4, runs=SATURATED_RUNS, body: int = 220,
                        sub: float = 0.05, seed: int = 1):
    """`fams` families in `genomes` genomes (genes listed genome by genome, a genome's genes in family order).  Every gene is its
    family's random body of `body` residues with `sub` substitutions per copy and, spliced into its middle, a stretch of
    runs[(family + genome) % len(runs)] repeats of the family's unit of `period` letters (letters family, family + 1, ...: no two
    families share a planted k-mer).  Runs stay at 3000: K-rle's cost is quadratic in the run length.
    -> pandelos_amd.synth.GeneSet"""
    assert 1 <= period < 20 and fams <= 20 and max(runs) <= 3000
    rng = np.random.default_rng(seed)
    bases = [LETTERS[rng.integers(0, 20, body)] for _ in range(fams)]
    genes, gen, fam_of = [], [], []
    for g in range(genomes):
        for f in range(fams):
            s = bases[f].copy()
            m = rng.random(body) < sub
            s[m] = LETTERS[rng.integers(0, 20, int(m.sum()))]
            unit = LETTERS[[(f + j) % 20 for j in range(period)]]
            genes.append(np.concatenate([s[:body // 2], stretch(unit, runs[(f + g) % len(runs)], k), s[body // 2:]]))
            gen.append(g); fam_of.append(f)
    return _as_gene_set(genes, gen, fam_of)


def saturated_dense_set(k: int = 3, genes: int = 600, genomes: int = 5, runs=(1022, 1023, 1100, 2500), first: int = 1, flank: int = 40, seed: int = 5):
    """One planted k-mer that EVERY gene holds (a stretch of the alphabet's last but one letter between two random flanks of
    `flank` residues, runs[(i + first) % len(runs)] occurrences in gene i): its rank-group has `genes` members, so gene i's one
    range of it holds genes - 1 - i postings.  The cycle starts at runs[first] = 1023, so that gene 0 — the group's head, the only
    record of the set whose count word ever carried the head bit AND is read again — has a saturated count.  Genes listed genome by
    genome.  -> pandelos_amd.synth.GeneSet"""
    rng = np.random.default_rng(seed)
    out = [np.concatenate([LETTERS[rng.integers(0, 20, flank)], stretch([ord("W")], runs[(i + first) % len(runs)], k), LETTERS[rng.integers(0, 20, flank)]])
           for i in range(genes)]
    per = -(-genes // genomes)
    return _as_gene_set(out, [i // per for i in range(genes)], [0] * genes)


def rank_groups(d):
    """The oracle's dictionary `d` (records {rank, seq, count}) -> (records in (rank, gene) order, group id of each, first record of
    each group, size of each group), with the groups as the reference's scan forms them: the globally last record never opens one
    (library.cpp:297-306), it belongs to the group in front of it."""
    o = np.lexsort((d["seq"], d["rank"]))
    r = d[o]
    new = np.r_[True, r["rank"][1:] != r["rank"][:-1]]
    if len(r) > 1:
        new[-1] = False
    gid = np.cumsum(new) - 1
    if len(r) > 1 and r["rank"][-1] != r["rank"][-2]:   # the folded record: its place inside the group is by gene
        o2 = np.lexsort((r["seq"], gid))
        r, gid = r[o2], gid[o2]
    start = np.flatnonzero(np.r_[True, gid[1:] != gid[:-1]])
    return r, gid, start, np.diff(np.r_[start, len(r)])


def fold_saturated_set(variant: str, k: int = 3, fams: int = 6, genomes: int = 3, body: int = 120, run: int = 3000, seed: int = 3):
    """The fold of the globally last record (library.cpp:300-306) meets a saturated count.  Bodies over the 19 letters below Y;
    the k-mers that start with Y are the largest ranks, and there are two of them: Y..Y, `run` times at the END of gene X and
    nowhere else (the globally last record, a singleton with a count of `run`), and the motif YA..AC in the middle of the genes of
    X's family in the other genomes (the group in front of it, into which the record is folded).  X's family is family 2.
      "head":   X is in genome 0: the folded record has the smallest gene id of the group and becomes its head
      "middle": X is in genome 1: the folded record lands between the members
      "same_gene_twice": as "middle", and X holds the motif too (the shape of the q1_fold_same_gene_twice fixture)
    -> (pandelos_amd.synth.GeneSet, id of gene X)"""
    rng = np.random.default_rng(seed)
    low = LETTERS[:19]
    motif = np.frombuffer(b"Y" + b"A" * (k - 2) + b"C", np.uint8)
    bases = [low[rng.integers(0, 19, body)] for _ in range(fams)]
    xg = 0 if variant == "head" else 1
    genes, gen, fam_of, x = [], [], [], -1
    for g in range(genomes):
        for f in range(fams):
            s = bases[f].copy()
            m = rng.random(body) < 0.05
            s[m] = low[rng.integers(0, 19, int(m.sum()))]
            if f == 2:
                with_motif = np.concatenate([s[:body // 2], motif, s[body // 2:]])
                if g != xg:
                    s = with_motif
                else:
                    x = len(genes)
                    s = np.concatenate([with_motif if variant == "same_gene_twice" else s, [low[0]], stretch([ord("Y")], run, k)])
            genes.append(s); gen.append(g); fam_of.append(f)
    return _as_gene_set(genes, gen, fam_of), x


class OracleCase:
    """A gene set with everything the CPU oracle says about it; made once, never changed."""

    def __init__(self, gs, k: int):
        from oracle import binding as ob
        ora = ob.Oracle(gs.residues, gs.offsets, gs.genome_of, k)
        self.gs, self.k, self.genomes = gs, k, int(ora.genomes)
        self.arrays = (gs.residues, gs.offsets, gs.genome_of)
        self.want = [ora.scores(g) for g in range(ora.genomes)]
        self.total_cost = int(ora.total_cost)
        self.genome_cost = [int(ora.genome_cost(g)) for g in range(ora.genomes)]
        self.dictionary, self.total_visited, self.kseq = ora.dictionary(), ora.total_visited(), ora.kseq_lengths()
        ora.close()


_CASES = {}


def saturated_case(name: str) -> OracleCase:
    """"sat:<k>:<period>" = saturated_count_set(k, period), "dense" = saturated_dense_set() at k = 3"""
    if name not in _CASES:
        kind, _, arg = name.partition(":")
        if kind == "sat":
            k, period = (int(x) for x in arg.split(":"))
            _CASES[name] = OracleCase(saturated_count_set(k, period), k)
        elif kind == "dense":
            _CASES[name] = OracleCase(saturated_dense_set(), 3)
        else:
            raise KeyError(name)
    return _CASES[name]
