"""Gene sets of 2^22 genes and more, each with everything the CPU oracle says about it.  At N >= 2^22 the library leaves its packed
forms (pdl_dict.hip range_plan, pdl_join.hip pack_ok / defer_wide / tier 0's `can`, pdl_query.h pack_ok: DESIGN.md section 3,
"Sets of 2^22 genes and more"); a 22-bit mask or a packed key on the wrong side of one of those switches swaps column c for
c - 2^22.  A gene shorter than k has no k-mer and costs a few words: all but about a thousand genes here are such FILLER, and a set
of 4.2 M genes builds and scores in the time of a small one.

Three genomes, k = 4, the 20-letter alphabet, real genes of 60 residues (57 k-mers, more than 2k: nothing but the missing packed
ranges keeps tier 0 away).  Filler is empty, or k - 1 times the letter A for every fourth id.  B = 2^22.

  genome 0   ids 0..23 one member of each of 24 small families, id 24 a member of family "mid", id 25 one of family "big", id 26 one
             of family "wave", then filler up to the first id of genome 1
  genome 1   LEAD members of mid and big by turns, then (at `s1 + LEAD`) one member of each small family j = 0..23 in order, one of
             each of two "high" families that genome 0 lacks, then 20 wave and the rest of 150 mid and 300 big
  genome 2   the small families in reversed order, the two high families, 20 wave, 150 mid, 300 big

so that mid has 301 members (rows of 300 cells: the 257-512 branch of order_wide_row), big 601 (rows of 600: its general network),
wave 41 (rows of 40: ranked by one wave), a small family 3 (rows of 2: the sub-wave rows), a high family 2: in "above" all its ids, and so
the label K-fam gives the family, are at or above B.  Substitution rate 4 % against the family's base.

  "above"   genome 1 starts at B - LEAD: its small family j is id B + j, while id j is family j's member in genome 0: id c and
            id c - B are both real and homologous to different rows.  500 filler genes lie between the two genomes' real genes: N = B + 1480.
  "at"      N == B: genomes 1 and 2 shifted down so that the last real gene is id B - 1, the set's last
  "below"   N == B - 1: the last packed size; its last gene, B - 2, is real
  "lift"    "below" cut to genomes 0 and 1 and shifted up: N = B - LIFT_UNDER.  `lift_query()` is a third genome of 40 real genes
            (one of each small family, 8 mid, 8 big); base + query has N = B + 40 - LIFT_UNDER.  case("lift") is the base's
            oracle, case("lift+") the union's.

  hub()     for the query's join, whose rows leave the LDS table only past QJ_LIMIT + QJ_T = 3840 columns (pdl_query.h) and which no
            option forces out: a base of genome 0 (27 real genes, filler up to B) and genome 1 = HUBS genes at ids B .., each 28
            random residues, the word HUB_WORD, 28 more; the query is three genes, the first a copy of hub 17 with 4 % substitutions
            and the word intact: its row meets every hub, all of them columns at or above B, in the HBM tables laid out by N + n.

Oracle blocks are made on first use and kept (a block of genome 0 walks 4.19 M rows: 12-14 s on the CPU; the other two take 0.2 s):
no test computes one twice."""
from __future__ import annotations

import functools

import numpy as np

from tests import helpers as H

K = 4
B = 1 << 22
GENE_LEN = 60
LEAD = 12                                                # real genes of genome 1 in front of its small families
SMALL, N_MID, N_BIG, N_WAVE = 24, 150, 300, 20           # small families; members of mid, big and wave in genomes 1 and 2, each
FILLER_LETTER = H.LETTERS[0]
SUB = 0.04
LIFT_UNDER = 5                                           # the "lift" base has N = B - LIFT_UNDER
LIFT_QUERY = (SMALL, 8, 8)                               # the genome to append: small families, mid, big
SIZES = ("below", "at", "above")
MID, BIG, WAVE = SMALL, SMALL + 1, SMALL + 2             # family numbers
HIGH = (SMALL + 3, SMALL + 4)
# K-order's branches by cells of a row (pdl_join.hip: ORDER_SUB_W, ORDER_WAVE_CELLS, order_wide_row's 257-512 and > 512)
ORDER_SUB_W, ORDER_WAVE_CELLS, ORDER_ONE_WORD_CELLS = 16, 256, 512


def _bases():
    rng = np.random.default_rng(2222)
    return [H.LETTERS[rng.integers(0, 20, GENE_LEN)] for _ in range(SMALL + 5)]


def _member(base, rng):
    s = base.copy()
    m = rng.random(len(s)) < SUB
    s[m] = H.LETTERS[rng.integers(0, 20, int(m.sum()))]
    return s


def _genome_families(genome: int):
    """family of every real gene of genome 1 or 2, in id order from the genome's first id"""
    if genome == 1:
        lead = [MID, BIG] * (LEAD // 2)
        return lead + list(range(SMALL)) + list(HIGH) + [WAVE] * N_WAVE + [MID] * (N_MID - LEAD // 2) + [BIG] * (N_BIG - LEAD // 2)
    return list(range(SMALL))[::-1] + list(HIGH) + [WAVE] * N_WAVE + [MID] * N_MID + [BIG] * N_BIG


REAL_1, REAL_2 = len(_genome_families(1)), len(_genome_families(2))


def _assemble(n_total: int, real: dict, genome_start):
    """n_total genes, `real`: {id: residues}, the rest filler; genome g starts at genome_start[g] -> GeneSet"""
    ids = np.arange(n_total, dtype=np.int64)
    length = np.where(ids % 4 == 1, K - 1, 0).astype(np.int64)
    rid = np.fromiter(real.keys(), np.int64, len(real))
    length[rid] = GENE_LEN
    offsets = np.zeros(n_total + 1, np.uint64)
    np.cumsum(length, out=offsets[1:])
    residues = np.full(int(offsets[-1]), FILLER_LETTER, np.uint8)
    for i, s in real.items():
        assert len(s) == GENE_LEN
        residues[int(offsets[i]):int(offsets[i]) + GENE_LEN] = s
    genome_of = (np.searchsorted(np.asarray(genome_start, np.int64), ids, side="right") - 1).astype(np.uint32)
    family = np.full(n_total, -1, np.int64)
    return residues, offsets, genome_of, family


def layout(n_total: int, genomes: int = 3):
    """(s1, s2): the first ids of genomes 1 and 2.  With room for it (n_total >= B - LEAD + REAL_1 + REAL_2, "above") genome 1
    starts at B - LEAD and genome 2's real genes end the set; smaller sets: the real genes of both end at the set's last id."""
    if genomes == 2:
        return n_total - REAL_1, n_total
    if n_total >= B - LEAD + REAL_1 + REAL_2:
        return B - LEAD, n_total - REAL_2
    return n_total - REAL_2 - REAL_1, n_total - REAL_2


N_ABOVE = B - LEAD + REAL_1 + 500 + REAL_2               # 500 filler genes between genomes 1's real genes and genome 2's
N_OF = {"below": B - 1, "at": B, "above": N_ABOVE, "lift": B - LIFT_UNDER}


@functools.lru_cache(maxsize=None)
def gene_set(n_total: int, genomes: int = 3):
    """the set of n_total genes in `genomes` genomes -> GeneSet; family_of is -1 for filler.  Made once, read-only"""
    from pandelos_amd.synth import GeneSet
    s1, s2 = layout(n_total, genomes)
    assert SMALL + 3 < s1 and s1 + REAL_1 <= s2 <= n_total
    bases, rng = _bases(), np.random.default_rng(n_total % 1000 + genomes)
    fam_at = {j: j for j in range(SMALL)}
    fam_at[SMALL], fam_at[SMALL + 1], fam_at[SMALL + 2] = MID, BIG, WAVE
    fam_at.update({s1 + i: f for i, f in enumerate(_genome_families(1))})
    if genomes == 3:
        fam_at.update({s2 + i: f for i, f in enumerate(_genome_families(2))})
    real = {i: _member(bases[f], rng) for i, f in sorted(fam_at.items())}
    residues, offsets, genome_of, family = _assemble(n_total, real, [0, s1, s2][:genomes])
    family[list(fam_at)] = list(fam_at.values())
    for a in (residues, offsets, genome_of, family):
        a.setflags(write=False)
    return GeneSet(residues, offsets, genome_of, family)


@functools.lru_cache(maxsize=None)
def lift_query():
    """(residues, offsets, family of each gene): the genome that lifts the "lift" base over B"""
    bases, rng = _bases(), np.random.default_rng(4040)
    fams = list(range(SMALL)) + [MID] * LIFT_QUERY[1] + [BIG] * LIFT_QUERY[2]
    genes = [_member(bases[f], rng) for f in fams]
    gs = H.as_gene_set(genes, [0] * len(genes), fams)
    return gs.residues, gs.offsets, np.asarray(fams, np.int64)


def _lift_union():
    from pandelos_amd.synth import GeneSet
    base = gene_set(N_OF["lift"], 2)
    rq, oq, fq = lift_query()
    return GeneSet(np.concatenate([base.residues, rq]).astype(np.uint8),
                   np.concatenate([base.offsets, base.offsets[-1] + oq[1:]]).astype(np.uint64),
                   np.concatenate([base.genome_of, np.full(len(fq), 2, np.uint32)]),
                   np.concatenate([base.family_of, fq]))


class _Blocks:
    """want[g]: the oracle's Scores block of genome g, made on first use and kept"""

    def __init__(self, ora):
        self._ora, self._got = ora, {}

    def __len__(self):
        return int(self._ora.genomes)

    def __getitem__(self, g):
        if not 0 <= g < len(self):
            raise IndexError(g)
        if g not in self._got:
            block = self._ora.scores(g)
            for v in block.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            self._got[g] = block
        return self._got[g]


class WideCase:
    """A set with what the CPU oracle says about it (the fields of helpers.OracleCase; `want` is lazy); never changed"""

    def __init__(self, gs, k: int):
        from oracle import binding as ob
        ora = ob.Oracle(gs.residues, gs.offsets, gs.genome_of, k)
        assert ora.status == 0
        self.gs, self.k, self.genomes, self.n = gs, k, int(ora.genomes), int(gs.genes)
        self.arrays = (gs.residues, gs.offsets, gs.genome_of)
        self.family = gs.family_of
        self.want = _Blocks(ora)
        self.total_cost = int(ora.total_cost)
        self.genome_cost = [int(ora.genome_cost(g)) for g in range(ora.genomes)]
        self.dictionary, self.total_visited, self.kseq = ora.dictionary(), ora.total_visited(), ora.kseq_lengths()
        self.first_id = [int(np.searchsorted(gs.genome_of, g)) for g in range(self.genomes)]

    @property
    def real(self):
        return np.flatnonzero(self.family >= 0)

    def small_ids(self, j: int):
        """ids of small family j's members, ascending: one per genome"""
        return np.flatnonzero(self.family == j)


@functools.lru_cache(maxsize=None)
def case(name: str) -> WideCase:
    """"below", "at", "above"; "lift" (two genomes, N < B) and "lift+" (with lift_query() as genome 2, N >= B)"""
    if name == "lift+":
        return WideCase(_lift_union(), K)
    return WideCase(gene_set(N_OF[name], 2 if name == "lift" else 3), K)


def base_and_query(c: WideCase, held: int):
    """((residues, offsets, genome_of) of the genomes below `held`, (residues, offsets) of genome `held`), `held` the last genome"""
    assert held == c.genomes - 1
    res, off, gen = c.arrays
    n = c.first_id[held]
    cut = int(off[n])
    return (res[:cut], off[:n + 1], gen[:n]), (res[cut:], (off[n:] - off[n]).astype(np.uint64))


HUBS = 4000
HUB_WORD = np.frombuffer(b"WYWC", dtype=np.uint8)
QUERY_MUST_LEAVE = 3840                                  # QJ_LIMIT + QJ_T of pdl_query.h: a row of as many distinct columns leaves the LDS table


@functools.lru_cache(maxsize=None)
def hub():
    """-> {"k", "base": (residues, offsets, genome_of), "query": (residues, offsets), "n": genes of the union, "want": the oracle's
    block of the query as genome 2 of the union, "genome_cost", "partners": ids of the genes that share a k-mer with query gene 0}"""
    from oracle import binding as ob
    rng = np.random.default_rng(1717)
    bases = _bases()
    real = {j: _member(bases[j], rng) for j in range(SMALL + 3)}
    hubs = [np.concatenate([H.LETTERS[rng.integers(0, 20, 28)], HUB_WORD, H.LETTERS[rng.integers(0, 20, 28)]]) for _ in range(HUBS)]
    real.update({B + i: h for i, h in enumerate(hubs)})
    q0 = _member(hubs[17], rng)
    q0[28:32] = HUB_WORD
    query = [q0, _member(bases[3], rng), H.LETTERS[rng.integers(0, 20, GENE_LEN)]]
    real.update({B + HUBS + i: q for i, q in enumerate(query)})
    n = B + HUBS + len(query)
    res, off, gen, _ = _assemble(n, real, [0, B, B + HUBS])
    ora = ob.Oracle(res, off, gen, K)
    assert ora.status == 0 and ora.genomes == 3
    want, cost, d = ora.scores(2), int(ora.genome_cost(2)), ora.dictionary()
    ora.close()
    r, gid, start, size = H.rank_groups(d)
    mine = gid[r["seq"] == B + HUBS]
    partners = np.unique(np.concatenate([r["seq"][start[g]:start[g] + size[g]] for g in mine.tolist()]))
    cut, nb = int(off[B + HUBS]), B + HUBS
    return {"k": K, "base": (res[:cut], off[:nb + 1], gen[:nb]), "query": (res[cut:], (off[nb:] - off[nb]).astype(np.uint64)), "n": n,
            "want": want, "genome_cost": cost, "partners": partners[partners != B + HUBS]}


def shared_groups(c: WideCase):
    """(groups of two records or more, the records in them) as the reference's scan forms the groups"""
    sizes = H.rank_groups(c.dictionary)[3]
    return int((sizes >= 2).sum()), int(sizes[sizes >= 2].sum())


def cells_per_row(block) -> np.ndarray:
    """cells of every row that has one, from a Scores block"""
    return np.unique(np.asarray(block["row"]), return_counts=True)[1]
