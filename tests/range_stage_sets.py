"""Small gene sets that reach the corner cases of the range stage's host side (pandelos_amd/csrc/pdl_dict.hip, "the range
stage"), each with everything the CPU oracle says about it.  k = 3, genes of 30-100 residues.

  lonely_genome   three genomes; the middle one is a single gene over letters no other gene uses, so none of its k-mers is
                  shared: the gene gets no range.  Its shard — a genome batch of its own, the rank that owns it alone — builds
                  ZERO ranges: buffers for max(count, 1), an empty inbox on the owner's side of the sender path.  The reference
                  folds the dictionary's last record into the group before it whatever its rank (library.cpp:300-306), which
                  would hand the gene a range if one of its records were the last or the one before: its letters (K L M) lie
                  in the middle of the alphabet, the other genes use both ends of it.
  one_range       two genes in two genomes that share exactly one k-mer, YYY at the end of both: the largest rank, so the last
                  record is a member of that group already and the fold has nothing to do.  One group of two records, one
                  upper range in the whole dictionary: of several ranks all but one make no tuple from their run, and a rank
                  of three owns no genome at all.

tests/test_range_stage_sets_cpu.py holds the sets to all that on the oracle; tests/test_gpu_range_stage.py runs them."""
from __future__ import annotations

import numpy as np

from tests import helpers as H

K = 3
LONELY_LETTERS = np.frombuffer(b"KLM", dtype=np.uint8)
OTHER_LETTERS = np.array([c for c in H.LETTERS if c not in LONELY_LETTERS], dtype=np.uint8)        # A..I and N..Y: both ends
LONELY_GENOME = 1
SETS = ("lonely_genome", "one_range")


def _lonely_genome(seed=7, fams=14, sub=0.08):
    rng = np.random.default_rng(seed)
    bases = [OTHER_LETTERS[rng.integers(0, len(OTHER_LETTERS), int(rng.integers(30, 101)))] for _ in range(fams)]
    genes, gen, fam = [], [], []
    for g in (0, 2):
        if g == 2:                                       # genome 1, between the two: the lonely gene
            genes.append(LONELY_LETTERS[rng.integers(0, len(LONELY_LETTERS), 60)]); gen.append(LONELY_GENOME); fam.append(fams)
        for f, base in enumerate(bases):                 # every family in both genomes: every other gene shares k-mers
            s = base.copy()
            m = rng.random(len(s)) < sub
            s[m] = OTHER_LETTERS[rng.integers(0, len(OTHER_LETTERS), int(m.sum()))]
            genes.append(s); gen.append(g); fam.append(f)
    return H._as_gene_set(genes, gen, fam)


def _distinct_kmers(letters, n):
    """n residues over `letters` in which no k-mer occurs twice (a walk that steps back from a k-mer it has seen)"""
    rng = np.random.default_rng(len(letters) * 1000 + n)
    while True:
        s = list(letters[rng.integers(0, len(letters), K - 1)])
        seen = set()
        while len(s) < n:
            options = [c for c in rng.permutation(letters) if bytes(s[-(K - 1):] + [c]) not in seen]
            if not options:
                break
            s.append(options[0]); seen.add(bytes(s[-K:]))
        if len(s) == n:
            return np.asarray(s, np.uint8)


def _one_range():
    tail = np.frombuffer(b"Y" * K, dtype=np.uint8)
    a = np.concatenate([_distinct_kmers(np.frombuffer(b"ACDEF", np.uint8), 40), tail])
    b = np.concatenate([_distinct_kmers(np.frombuffer(b"GHIKL", np.uint8), 55), tail])
    return H._as_gene_set([a, b], [0, 1], [0, 0])


_CACHE = {}


def case(name) -> H.OracleCase:
    """The set and the oracle's answer; made once, never changed."""
    if name not in _CACHE:
        _CACHE[name] = H.OracleCase({"lonely_genome": _lonely_genome, "one_range": _one_range}[name](), K)
    return _CACHE[name]


def shared_groups(c: H.OracleCase):
    """(groups of two records or more, the records in them) as the reference's scan forms the groups"""
    sizes = H.rank_groups(c.dictionary)[3]
    return int((sizes >= 2).sum()), int(sizes[sizes >= 2].sum())


def lonely_gene(c: H.OracleCase) -> int:
    ids = np.flatnonzero(c.gs.genome_of == LONELY_GENOME)
    assert len(ids) == 1
    return int(ids[0])
