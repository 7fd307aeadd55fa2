"""Small gene sets that reach every branch of the best-hit filter (K-bbh, pandelos_amd/csrc/pdl_bbh.hip), a count of which
branches a Scores block reaches, and a restatement of the filter in which one condition at a time can be altered.

make_gene_set gives a family at most two copies per genome and, wherever paralogs exist, no exact copies across genomes: its
sets hold no best hit at 1.0 next to an intra-genome cell, no intra cell that is its row's best but not its column's, and hardly a
mutual best pair at its row's threshold.  The sets here are built the other way round: some families are identical in every
genome (best hits at exactly 1.0), and a genome's copy of a family is followed by a chain of paralogs, each mutated off the one
before it at a rate that may be 0 (exact duplicates: ties) or large (a chain's far end is the best of its neighbour only).

The seeds below were chosen on the CPU oracle (search_seeds) so that every event of FLOORS occurs and every variant of VARIANTS
gives another edge list; a mutual best pair exactly at its row's threshold is too rare to search for inside one genome's block,
so "single" and "batch" plant one (_planted_pair).  tests/test_bbh_branches_cpu.py holds the sets to all that."""
from __future__ import annotations

import numpy as np

from tests import helpers as H

K = 3
INT32_MAX = int(np.iinfo(np.int32).max)
PARALOG_RATES = (0.0, 0.03, 0.08, 0.2)            # a paralog against the copy in front of it
MAX_GENES, MAX_CELLS = 200, 1500

# name -> the arguments of make_set: families (seed, count, mean length, share that is identical in every genome), substitution
# rate of a genome's copy of the other families, presence, one seed per genome; `chains` and `planted` as make_set says
SETS = {
    "chains": dict(fam_seed=100, fams=24, length=60, identical=0.3, sub=0.12, presence=0.9, genome_seeds=(1000, 1001, 1002, 1014)),
    "identical2": dict(fam_seed=200, fams=24, length=60, identical=1.0, sub=0.0, presence=1.0, genome_seeds=(2000, 2001)),
    "single": dict(fam_seed=300, fams=15, length=60, identical=0.3, sub=0.12, presence=0.9, genome_seeds=(3000, 3001, 3002, 3003),
                   chains=(0.5, 0.5, 0.5, 1.0), planted=(3, 4)),
    "batch": dict(fam_seed=300, fams=15, length=60, identical=0.3, sub=0.12, presence=0.9, genome_seeds=(3000, 3001, 3002, 3003, 3098),
                  chains=(0.5, 0.5, 0.5, 1.0, 1.0), planted=(3, 4)),
}
# genomes whose block alone reaches every branch: in "single" the last genome in the set as it is; in "batch" each of the last two
# in the set made of the first three genomes and itself (what a query of that genome against those three sees).  "single" is
# "batch" without its last genome.
ALL_BRANCHES = {"single": (3,), "batch": (3, 4)}
BATCH_BASE = (0, 1, 2)


def _mutated(rng, s, rate):
    s = s.copy()
    m = rng.random(len(s)) < rate
    s[m] = H.LETTERS[rng.integers(0, 20, int(m.sum()))]
    return s


def _families(fam_seed, fams, length, identical):
    rng = np.random.default_rng(fam_seed)
    bases = [H.LETTERS[rng.integers(0, 20, int(rng.integers(length - 15, length + 16)))] for _ in range(fams)]
    return bases, rng.random(fams) < identical


PLANTED_LENGTH = 90


def _planted_pair(rng, text):
    """(X, X2): `text` with one substitution, and X with one more, far from the first.  A substitution inside a gene takes K k-mers
    away, so X shares as many k-mers with `text` as with X2, and all three are equally long: score(X, text) == score(X, X2) to the
    bit.  `text` is longer than every family, so with it in one other genome alone, score(X, text) is the largest best hit below 1
    toward that genome and the only threshold X has: the pair (X, X2) sits exactly at its row's threshold."""
    x = text.copy()
    p = int(rng.integers(10, 40))
    x[p] = H.LETTERS[(int(np.searchsorted(H.LETTERS, x[p])) + int(rng.integers(1, 20))) % 20]
    x2 = x.copy()
    p = int(rng.integers(50, 80))
    x2[p] = H.LETTERS[(int(np.searchsorted(H.LETTERS, x2[p])) + int(rng.integers(1, 20))) % 20]
    return x, x2


def _genome(seed, bases, same, sub, presence, chains=0.5):
    """One genome's genes: per present family its copy (the family's text itself where the family is identical everywhere), and
    behind a share `chains` of the copies a chain of 1-3 paralogs."""
    rng = np.random.default_rng(seed)
    genes, fam = [], []
    for f, base in enumerate(bases):
        if rng.random() >= presence:
            continue
        s = base if same[f] else _mutated(rng, base, sub)
        genes.append(s); fam.append(f)
        if rng.random() < chains:
            for _ in range(int(rng.integers(1, 4))):
                s = _mutated(rng, s, PARALOG_RATES[int(rng.integers(0, len(PARALOG_RATES)))])
                genes.append(s); fam.append(f)
    return genes, fam


def make_set(fam_seed, fams, length, identical, sub, presence, genome_seeds, chains=None, planted=()):
    """-> pandelos_amd.synth.GeneSet, genes listed genome by genome.  `chains`: per genome, the share of copies followed by paralogs.
    `planted`: the genomes that end with a pair at its row's threshold (_planted_pair); the j-th of them has it of a text of its
    own, which genome j ends with (a genome listed here that the set does not have leaves its text behind all the same)."""
    bases, same = _families(fam_seed, fams, length, identical)
    texts = [H.LETTERS[np.random.default_rng(fam_seed + 1 + j).integers(0, 20, PLANTED_LENGTH)] for j in range(len(planted))]
    genes, gen, fam = [], [], []
    for g, seed in enumerate(genome_seeds):
        gg, ff = _genome(seed, bases, same, sub, presence, 0.5 if chains is None else chains[g])
        if g < len(planted):
            gg.append(texts[g]); ff.append(fams + g)
        if g in planted:
            j = planted.index(g)
            gg += list(_planted_pair(np.random.default_rng(seed + 1), texts[j])); ff += [fams + j] * 2
        genes += gg; fam += ff; gen += [g] * len(gg)
    return H._as_gene_set(genes, gen, fam)


def subset(gs, genomes):
    """The genes of `genomes` (ascending) as a set of their own, genome ids renumbered 0.. in that order."""
    off = gs.offsets.astype(np.int64)
    new = {g: i for i, g in enumerate(genomes)}
    ids = [i for i in range(gs.genes) if int(gs.genome_of[i]) in new]
    return H._as_gene_set([gs.residues[off[i]:off[i + 1]] for i in ids], [new[int(gs.genome_of[i])] for i in ids], [int(gs.family_of[i]) for i in ids])


_CACHE = {}


def gene_set(name):
    if ("set", name) not in _CACHE:
        _CACHE["set", name] = make_set(**SETS[name])
    return _CACHE["set", name]


def oracle_blocks(gs, k=K):
    """The CPU oracle's Scores blocks of a set, one dict per genome."""
    from oracle import binding as ob
    ora = ob.Oracle(gs.residues, gs.offsets, gs.genome_of, k)
    out = [ora.scores(g) for g in range(ora.genomes)]
    ora.close()
    return out


def blocks(name, genomes=None):
    """Oracle blocks of set `name` (made once, never changed), or of its subset of `genomes`."""
    key = ("blocks", name, None if genomes is None else tuple(genomes))
    if key not in _CACHE:
        _CACHE[key] = oracle_blocks(gene_set(name) if genomes is None else subset(gene_set(name), list(genomes)))
    return _CACHE[key]


def all_branch_blocks(name):
    """[(label, block)] of the blocks that must reach every branch alone."""
    if name == "single":
        return [("single genome 3", blocks("single")[3])]
    return [(f"batch base + genome {q}", blocks("batch", BATCH_BASE + (q,))[len(BATCH_BASE)]) for q in ALL_BRANCHES["batch"]]


# ---- the filter, restated ---------------------------------------------------------------------------------------------------
VARIANTS = (
    "no_below_1",          # :116  inter_max_score takes every best hit, 1.0 included
    "at_most_1",           # :116  score <= 1.0 for score < 1.0
    "p1_no_column_best",   # :101  phase 1 without the column's best
    "p1_no_row_best",      # :100  phase 1 without the row's best
    "thr_default_0",       # :147  scoresRowThreshold starts at 0, not +inf
    "thr_max",             # :153  the largest inter_max_score of the row's best-hit genomes, not the smallest
    "thr_by_column",       # :153  the threshold filed under the column gene
    "p2_no_column_best",   # :169  phase 2 without the column gene's best inside the genome
    "p2_no_row_best",      # :168  phase 2 without the row gene's best inside the genome
    "greater",             # :170  > for >=
    "no_threshold",        # :170  no threshold test
    "row_not_column",      # :165  row != column for row < column
)


def _fields(block):
    if isinstance(block, dict):
        return block
    return {f: getattr(block, f) for f in ("scoresCount",) + H.FIELDS}


def filter_cells(block, variant=""):
    """Pangenes.java:98-176 on one Scores block -> (cells of phase 1, cells of phase 2), each a list of cell indices in the order
    the loops meet them.  A phase-1 cell adds (row, column) and (column, row) (:103-104), a phase-2 cell (row, column) (:174).
    `variant` (one of VARIANTS) alters exactly one condition."""
    assert variant == "" or variant in VARIANTS, variant
    b = _fields(block)
    n = int(b["scoresCount"])
    score, row, col = b["scores"], b["row"], b["column"]
    g1, g2 = b["first_seq_genome"], b["second_seq_genome"]
    best, col_best, at = b["max_genome_score"], b["max_genome_score_col"], b["scoresMaxMappings"]
    genomes = best.shape[1] if best.ndim == 2 else 0
    one, inf = np.float32(1.0), np.float32(np.inf)
    inter_max = [np.float32(0.0)] * genomes                                    # :72
    added = [False] * n                                                        # :96
    phase1 = []
    for i in range(n):                                                         # :98
        if g1[i] == g2[i]:                                                     # :99
            continue
        is_row_best = variant == "p1_no_row_best" or score[i] == best[at[row[i]]][g2[i]]          # :100
        is_col_best = variant == "p1_no_column_best" or score[i] == col_best[col[i]]              # :101
        if not (is_row_best and is_col_best):
            continue
        phase1.append(i)                                                       # :103-104
        added[i] = True                                                        # :106
        sg = int(g2[i])                                                        # :108
        below = True if variant == "no_below_1" else score[i] <= one if variant == "at_most_1" else score[i] < one
        if below and score[i] > inter_max[sg]:                                 # :116
            inter_max[sg] = score[i]                                           # :117
    start = np.float32(0.0) if variant == "thr_default_0" else inf
    thr, seen = {}, set()                                                      # :146-147 (a missing key is the initial value)
    for i in range(n):                                                         # :149
        if not added[i]:                                                       # :150
            continue
        key = int(col[i]) if variant == "thr_by_column" else int(row[i])       # :151
        v = inter_max[int(g2[i])]                                              # :152
        if variant == "thr_max":
            thr[key] = max(thr[key], v) if key in seen else v
        else:
            thr[key] = min(thr.get(key, start), v)                             # :153
        seen.add(key)
    phase2 = []
    for i in range(n):                                                         # :164
        ordered = row[i] != col[i] if variant == "row_not_column" else row[i] < col[i]            # :165
        if not ordered or g1[i] != g2[i]:                                      # :167
            continue
        if variant != "p2_no_row_best" and score[i] != best[at[row[i]]][g2[i]]:                   # :168
            continue
        if variant != "p2_no_column_best" and score[i] != best[at[col[i]]][g2[i]]:                # :169
            continue
        t = thr.get(int(row[i]), start)
        if variant == "no_threshold" or (score[i] > t if variant == "greater" else score[i] >= t):    # :170
            phase2.append(i)                                                   # :174
    return phase1, phase2


def edges_of_cells(block, cells):
    """(phase-1 cells, phase-2 cells) -> (src, dst, score) in insertion order, as pangenes.bbh_edges returns them."""
    b = _fields(block)
    p1, p2 = (np.asarray(c, np.int64) for c in cells)
    row, col, score = b["row"].astype(np.int64), b["column"].astype(np.int64), b["scores"]
    src = np.empty(2 * len(p1), np.int64); dst = np.empty(2 * len(p1), np.int64); sc = np.empty(2 * len(p1), np.float32)
    src[0::2], dst[0::2], sc[0::2] = row[p1], col[p1], score[p1]
    src[1::2], dst[1::2], sc[1::2] = col[p1], row[p1], score[p1]
    return np.concatenate([src, row[p2]]), np.concatenate([dst, col[p2]]), np.concatenate([sc, score[p2]])


# ---- which branches a block reaches -----------------------------------------------------------------------------------------
EVENTS = ("inter_cells", "best_hits", "best_hits_at_1", "p1_row_best_only", "p1_column_best_only", "genomes_inter_max_0",
          "rows_thr_of_distinct_inter_max", "row_genome_pairs_with_tied_best_hits", "intra_cells", "intra_row_above_column",
          "p2_row_best_only", "p2_column_best_only", "mutual_kept", "mutual_kept_thr_0", "mutual_dropped_thr_inf",
          "mutual_dropped_below_thr", "mutual_equal_thr")


def events(block):
    """Counts, for one Scores block, of the cells and rows at which the filter's conditions part.  The mutual_* counts are of
    intra-genome cells with row < column that are the best of both genes; mutual_equal_thr is part of mutual_kept."""
    b = _fields(block)
    n = int(b["scoresCount"])
    score, row, col = b["scores"], b["row"], b["column"]
    g1, g2 = b["first_seq_genome"], b["second_seq_genome"]
    best, col_best, at = b["max_genome_score"], b["max_genome_score_col"], b["scoresMaxMappings"]
    genomes = best.shape[1] if best.ndim == 2 else 0
    ev = dict.fromkeys(EVENTS, 0)
    inter_max = [np.float32(0.0)] * genomes
    hit_genomes, hits = set(), {}
    for i in range(n):
        if g1[i] == g2[i]:
            continue
        ev["inter_cells"] += 1
        rb, cb = score[i] == best[at[row[i]]][g2[i]], score[i] == col_best[col[i]]
        ev["p1_row_best_only"] += int(rb and not cb)
        ev["p1_column_best_only"] += int(cb and not rb)
        if rb and cb:
            ev["best_hits"] += 1
            ev["best_hits_at_1"] += int(score[i] == np.float32(1.0))
            sg = int(g2[i])
            hit_genomes.add(sg)
            hits.setdefault(int(row[i]), []).append(sg)
            if score[i] < np.float32(1.0) and score[i] > inter_max[sg]:
                inter_max[sg] = score[i]
    ev["genomes_inter_max_0"] = sum(1 for sg in hit_genomes if inter_max[sg] == 0)
    thr = {}
    for r, sgs in hits.items():
        values = {float(inter_max[sg]) for sg in sgs}
        thr[r] = np.float32(min(values))
        ev["rows_thr_of_distinct_inter_max"] += int(len(values) > 1)
        ev["row_genome_pairs_with_tied_best_hits"] += sum(1 for sg in set(sgs) if sgs.count(sg) > 1)
    for i in range(n):
        if g1[i] != g2[i]:
            continue
        ev["intra_cells"] += 1
        if row[i] > col[i]:
            ev["intra_row_above_column"] += 1
        if row[i] >= col[i]:
            continue
        rb, cb = score[i] == best[at[row[i]]][g2[i]], score[i] == best[at[col[i]]][g2[i]]
        ev["p2_row_best_only"] += int(rb and not cb)
        ev["p2_column_best_only"] += int(cb and not rb)
        if not (rb and cb):
            continue
        t = thr.get(int(row[i]))
        if t is None:
            ev["mutual_dropped_thr_inf"] += 1
        elif score[i] < t:
            ev["mutual_dropped_below_thr"] += 1
        else:
            ev["mutual_kept"] += 1
            ev["mutual_kept_thr_0"] += int(t == 0)
            ev["mutual_equal_thr"] += int(score[i] == t)
    return ev


def sum_events(blks):
    tot = dict.fromkeys(EVENTS, 0)
    for blk in blks:
        for name, v in events(blk).items():
            tot[name] += v
    return tot


# Floors: conditions on the sets, not measurements of them.  Every event the variants turn on occurs three times or more; a mutual
# best pair exactly at its row's threshold is rare and has to occur once.
FLOORS = {name: 3 for name in EVENTS if name not in ("inter_cells", "intra_cells", "genomes_inter_max_0", "mutual_kept_thr_0")}
FLOORS["mutual_equal_thr"] = 1
FLOORS_IDENTICAL2 = {"best_hits_at_1": 3, "genomes_inter_max_0": 2, "mutual_kept_thr_0": 3}


def killed_by(blks):
    """-> {variant: indices of the blocks on which it gives other cells than the filter}"""
    return {v: [i for i, blk in enumerate(blks) if filter_cells(blk, v) != filter_cells(blk)] for v in VARIANTS}


def kill_table():
    """The table of DESIGN.md: per set, and per block that stands alone, the genomes whose block tells each variant from the filter."""
    rows = [("variant", "chains", "identical2", "single", "single, genome 3 alone", "batch", "batch, base + 3", "batch, base + 4")]
    cols = [killed_by(blocks("chains")), killed_by(blocks("identical2")), killed_by(blocks("single")),
            killed_by([blocks("single")[3]]), killed_by(blocks("batch"))] + [killed_by([blk]) for _, blk in all_branch_blocks("batch")]
    for v in VARIANTS:
        rows.append((f"`{v}`",) + tuple((",".join(map(str, c[v])) if j not in (3, 5, 6) else ("yes" if c[v] else "no")) or "-" for j, c in enumerate(cols)))
    return "\n".join("| " + " | ".join(r) + " |" + ("\n|" + "---|" * len(r) if i == 0 else "") for i, r in enumerate(rows))


def search_seeds(name, tries=200):
    """How the seeds of SETS were found: the first seed of the last genome (for "identical2", of the families) with which the
    floors hold and every variant is killed where it has to be.  Not run by the tests."""
    spec = dict(SETS[name])
    for t in range(tries):
        if name == "identical2":
            spec["fam_seed"] = SETS[name]["fam_seed"] + t
        else:
            spec["genome_seeds"] = SETS[name]["genome_seeds"][:-1] + (SETS[name]["genome_seeds"][-1] + t,)
        gs = make_set(**spec)
        blks = oracle_blocks(gs)
        if gs.genes > MAX_GENES or sum(int(b["scoresCount"]) for b in blks) > MAX_CELLS:
            continue
        if name == "batch":                                # (the last genome as a query against the base sees the base and itself)
            blks = oracle_blocks(subset(gs, list(BATCH_BASE) + [len(spec["genome_seeds"]) - 1]))
        if name == "identical2":
            tot = sum_events(blks)
            if all(tot[e] >= f for e, f in FLOORS_IDENTICAL2.items()) and tot["best_hits"] == tot["best_hits_at_1"]:
                return spec
            continue
        scope = blks if name == "chains" else blks[-1:]
        tot = sum_events(scope)
        if all(tot[e] >= f for e, f in FLOORS.items()) and all(killed_by(scope).values()):
            return spec
    return None
