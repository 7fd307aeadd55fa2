"""Cases of the genome-by-genome shared-family matrices (pdl_genome_matrix; pandelos_amd/csrc/pdl_matrix.h), their seeded generators,
the kernel's regime constants and two references that share no code: one with sets and ``Counter``s per genome pair
(``matrices_sets``: the contract read aloud), one with numpy over the labelling (``matrices_numpy``: ``P.T @ P`` in int64 and
``np.minimum`` per genome column).  ``stacked_bits`` restates the device's bit layout on the host.  test_matrix_cpu.py holds all of
them against each other and against ``pangenome.genome_matrix_host``; test_gpu_matrix.py holds the device against them."""
from __future__ import annotations

from collections import Counter
from functools import lru_cache

import numpy as np

from tests import profile_cases as PC

TILE = 64                 # genomes of one side of a workgroup's output tile (MX_TILE)
WORD = 64                 # bit columns of one word of a genome's row
KSTEP = 16                # words of a genome staged per step (MX_KSTEP)
MIN_SPLIT_WORDS = 32      # a k-split keeps at least so many words (MX_MIN_SPLIT_WORDS)
DEFAULT_SLAB_BYTES = 1 << 28
G_EDGES = (63, 64, 65, 128, 129)
F_EDGES = (1, 63, 64, 65, 129)


# ---- references ---------------------------------------------------------------------------------------------------------------
def matrices_sets(family_of, genome_of, G: int) -> dict:
    """The contract, genome pair by genome pair: the families two genomes both have a gene of; the smaller copy number, summed."""
    per_genome = [Counter() for _ in range(G)]
    for lab, g in zip(np.asarray(family_of).tolist(), np.asarray(genome_of).tolist()):
        per_genome[g][lab] += 1
    shared = [[len(set(a) & set(b)) for b in per_genome] for a in per_genome]
    copies = [[sum(min(n, b[lab]) for lab, n in a.items() if lab in b) for b in per_genome] for a in per_genome]
    return {"shared": np.array(shared, np.uint32).reshape(G, G), "shared_copies": np.array(copies, np.uint32).reshape(G, G)}


def matrices_numpy(family_of, genome_of, G: int) -> dict:
    """The same from a dense family x genome count table made of the labelling itself."""
    labs, inv = np.unique(np.asarray(family_of), return_inverse=True)
    table = np.zeros((len(labs), G), np.int64)
    np.add.at(table, (inv, np.asarray(genome_of, np.int64)), 1)
    P = (table > 0).astype(np.int64)
    shared_copies = np.empty((G, G), np.int64)
    for g in range(G):
        shared_copies[g] = np.minimum(table[:, g][:, None], table).sum(axis=0)
    return {"shared": (P.T @ P).astype(np.uint32), "shared_copies": shared_copies.astype(np.uint32)}


def first_difference(got: dict, want: dict):
    """-> None, or a sentence that names the first wrong (g, h)."""
    for n in ("shared", "shared_copies"):
        a, b = np.asarray(got[n]), np.asarray(want[n])
        if a.shape != b.shape:
            return f"{n}: shape {a.shape}, expected {b.shape}"
        bad = np.argwhere(a != b)
        if len(bad):
            g, h = bad[0].tolist()
            return f"{n}[{g}][{h}]: {int(a[g, h])}, expected {int(b[g, h])} ({len(bad)} elements differ)"
    return None


# ---- the device's layout, restated ---------------------------------------------------------------------------------------------
def layout(profile: dict) -> dict:
    """extra[f] = the largest copy count of family f - 1, extra_off its exclusive scan, E its sum; P = 64 * ceil(F / 64) presence
    columns, L = P + E levels, W = ceil(L / 64) words per genome."""
    F = int(profile["families"])
    off = profile["genome_off"].astype(np.int64)
    extra = np.maximum.reduceat(profile["copies"].astype(np.int64), off[:-1]) - 1
    extra_off = np.cumsum(extra) - extra
    P, E = WORD * -(-F // WORD), int(extra.sum())
    return dict(F=F, P=P, E=E, L=P + E, W=-(-(P + E) // WORD), extra=extra, extra_off=extra_off)


def stacked_bits(profile: dict) -> np.ndarray:
    """(G, L) bool, genome-major: bit f (f < F) of row g — family f has a gene in g; bit P + extra_off[f] + t - 2 — it has at
    least t of them, t >= 2."""
    lay = layout(profile)
    bits = np.zeros((int(profile["n_genomes"]), lay["L"]), bool)
    off = profile["genome_off"].tolist()
    for f in range(lay["F"]):
        for i in range(off[f], off[f + 1]):
            g, cp = int(profile["genomes"][i]), int(profile["copies"][i])
            bits[g, f] = True
            start = lay["P"] + int(lay["extra_off"][f])
            bits[g, start:start + cp - 1] = True
    return bits


def slab_plan(profile: dict, slab_bytes: int = DEFAULT_SLAB_BYTES) -> list:
    """The word ranges [w0, w1) the call works through: at most slab_bytes / (G * 8) words each (at least one), cut at P / 64."""
    lay = layout(profile)
    words = min(max(slab_bytes // (int(profile["n_genomes"]) * 8), 1), lay["W"])
    out = []
    for a, e in ((0, lay["P"] // WORD), (lay["P"] // WORD, lay["W"])):
        out += [(w0, min(w0 + words, e)) for w0 in range(a, e, words)]
    return out


def split_plan(slab_words: int, G: int, cus: int = 256) -> tuple:
    """-> (k-splits of a slab, words per split): workgroups for twice the CUs while a split keeps MIN_SPLIT_WORDS words, whole
    k-steps per split.  For one pair of tiles and slabs below cus * MIN_SPLIT_WORDS words the CU count does not come into it."""
    tiles = -(-G // TILE)
    pairs = tiles * (tiles + 1) // 2
    splits = max(1, min(-(-2 * cus // pairs), slab_words // MIN_SPLIT_WORDS))
    per = -(-(-(-slab_words // splits)) // KSTEP) * KSTEP
    return -(-slab_words // per), per


# ---- labellings ---------------------------------------------------------------------------------------------------------------
def from_copies(table) -> tuple:
    """A (families, genomes) table of copy counts (no empty row) -> (family_of, genome_of, G), the genes family by family."""
    table = np.asarray(table, np.int64)
    assert (table.sum(axis=1) > 0).all()
    f, g = np.nonzero(table)
    fam, gen = np.repeat(f, table[f, g]), np.repeat(g, table[f, g])
    first = np.r_[0, np.flatnonzero(np.diff(fam)) + 1]
    return first[fam].astype(np.uint32), gen.astype(np.uint32), table.shape[1]     # a family's label: its first gene


def random_copies(G: int, families: int, seed: int, density: float = 0.3, max_copies: int = 3, p_multi: float = 0.15) -> tuple:
    """Every family in about density * G genomes (at least one); where present, 1 copy, or with p_multi 2..max_copies."""
    rng = np.random.default_rng(seed)
    present = rng.random((families, G)) < density
    present[np.arange(families), rng.integers(0, G, families)] |= ~present.any(axis=1)
    more = (rng.random((families, G)) < p_multi) * rng.integers(1, max(2, max_copies), (families, G)) if max_copies > 1 else 0
    return from_copies(present * (1 + more))


@lru_cache(maxsize=None)
def matrix_cases() -> dict:
    """name -> (family_of, genome_of, G)."""
    rng = np.random.default_rng(21)
    singles = np.zeros((40, 5), np.int64)
    singles[np.arange(40), np.arange(40) % 5] = 1
    cases = {
        "one genome, one family": from_copies([[1]]),
        "two genomes": from_copies([[1, 1], [2, 0], [0, 1]]),
        "all singletons": from_copies(singles),
        "one family of everything": from_copies([[2, 1, 3, 1, 1]]),
        "a genome without a gene": from_copies([[1, 1, 0, 2], [0, 3, 0, 1], [1, 0, 0, 0]]),
        "copies (3, 1, 2)": from_copies([[3, 1, 2], [1, 0, 1], [0, 2, 2]]),
        "200 copies in one genome": from_copies([[200, 1, 1, 1], [1, 1, 0, 0], [2, 0, 1, 0]]),
        "70 copies from the last bit of a word": from_copies([[64, 1, 0], [70, 1, 1], [1, 2, 0]]),
        "copies >= 2 everywhere": from_copies(rng.integers(2, 5, (70, 6))),
    }
    for G in G_EDGES:
        cases[f"G = {G}"] = random_copies(G, 150, seed=G)
    cases["1025 genomes"] = random_copies(1025, 300, seed=1025, density=0.2)
    for F in F_EDGES:
        cases[f"F = {F}, single copies"] = random_copies(5, F, seed=F, density=0.5, max_copies=1)
        cases[f"F = {F}, with extras"] = random_copies(5, F, seed=100 + F, density=0.5, max_copies=4, p_multi=0.4)
    cases["slabs"] = random_copies(10, 200, seed=7, density=0.5, max_copies=4, p_multi=0.5)
    cases["k-split, 64 genomes"] = random_copies(64, 8000, seed=8, density=2.5 / 64, max_copies=3, p_multi=0.1)
    cases["k-split, short last part"] = random_copies(64, 6250, seed=9, density=2 / 64, max_copies=1)
    for G in (7, 64, 130):
        cases[f"random, {G} genomes"] = PC.random_labelling(G, genes=20000, genomes=G)
    cases["9 genomes"] = PC.random_labelling(100, genes=3000, genomes=9)
    return cases


SLAB_BYTES = 10 * 8 * 3          # of the case "slabs": three words of its ten genomes


@lru_cache(maxsize=None)
def expected(name: str) -> tuple:
    """-> (the profile, the matrices): made once, shared by the tests, left unchanged."""
    f, g, G = matrix_cases()[name]
    return PC.profile_numpy(f, g, G), matrices_numpy(f, g, G)


def small(name: str) -> bool:
    """Cases the pair-by-pair reference walks in a moment."""
    f, _, G = matrix_cases()[name]
    return len(f) <= 4000 and G <= 130
