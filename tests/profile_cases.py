"""Cases of the pan-genome profile (pdl_family_profile, pdl_pan_curves; pandelos_amd/csrc/pdl_profile.h), their seeded generators
and two references that share no code: one with Python sets and dicts (``profile_sets``, ``curves_sets``: the contract read
aloud), one with numpy (``profile_numpy``, ``curves_numpy``: sorted keys, accumulated presence).  test_profile_cpu.py holds them
against each other and against ``pangenome.pan_curves_host``; test_gpu_profile.py holds the device against them."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

G_EDGES = (1, 2, 63, 64, 65, 128, 129)              # around the words of the presence bits
BIG_FAMILIES = (255, 256, 257, 2048, 2049, 8193)    # around the tiles of the scan (2048) and of the sort (4096)
PAN_TILE = 2048                                     # families of one workgroup of k_pan_curves
ARRAYS = ("label", "size", "spread", "genome_off", "genomes", "copies", "size_hist", "spread_hist", "spread_by_genome",
          "genome_genes", "genome_core", "genome_accessory", "genome_unique")
COUNTS = ("n_sequences", "n_genomes", "families", "incidences", "max_size", "core", "single_copy_core", "unique", "accessory")


# ---- references ---------------------------------------------------------------------------------------------------------------
def profile_sets(family_of, genome_of, G: int) -> dict:
    """The contract with sets and dicts, gene by gene."""
    members = {}
    for gene, lab in enumerate(np.asarray(family_of).tolist()):
        members.setdefault(lab, []).append(gene)
    gen = np.asarray(genome_of).tolist()
    out = {n: [] for n in ("label", "size", "spread", "genomes", "copies")}
    out["genome_off"] = [0]
    size_hist, spread_hist = {}, [0] * (G + 1)
    by_genome = [[0] * G for _ in range(G + 1)]
    per_genome = {n: [0] * G for n in ("genome_genes", "genome_core", "genome_accessory", "genome_unique")}
    counts = dict(core=0, single_copy_core=0, unique=0, accessory=0)
    for lab in sorted(members):
        copies = {}
        for gene in members[lab]:
            copies[gen[gene]] = copies.get(gen[gene], 0) + 1
        size, spread = len(members[lab]), len(copies)
        out["label"].append(lab); out["size"].append(size); out["spread"].append(spread)
        for g in sorted(copies):
            out["genomes"].append(g); out["copies"].append(copies[g])
            by_genome[spread][g] += 1
            per_genome["genome_genes"][g] += copies[g]
            if spread == G:
                per_genome["genome_core"][g] += copies[g]
            if spread == 1:
                per_genome["genome_unique"][g] += copies[g]
            if spread != G and spread != 1:
                per_genome["genome_accessory"][g] += copies[g]
        out["genome_off"].append(len(out["genomes"]))
        size_hist[size] = size_hist.get(size, 0) + 1
        spread_hist[spread] += 1
        counts["core"] += spread == G
        counts["single_copy_core"] += spread == G == size
        counts["unique"] += spread == 1
        counts["accessory"] += spread != G and spread != 1
    max_size = max(size_hist)
    out["size_hist"] = [size_hist.get(s, 0) for s in range(max_size + 1)]
    out["spread_hist"], out["spread_by_genome"] = spread_hist, by_genome
    out.update(per_genome)
    out = {n: np.array(v, np.uint32) for n, v in out.items()}
    out.update(counts, n_sequences=len(gen), n_genomes=G, families=len(members), incidences=len(out["genomes"]), max_size=max_size)
    return out


def profile_numpy(family_of, genome_of, G: int) -> dict:
    """The same from unique (label, genome) keys."""
    fam, gen = np.asarray(family_of, np.int64), np.asarray(genome_of, np.int64)
    keys, copies = np.unique(fam * G + gen, return_counts=True)
    inc_label, genomes = keys // G, keys % G
    label, first, spread = np.unique(inc_label, return_index=True, return_counts=True)
    size = np.add.reduceat(copies, first)
    inc_spread = np.repeat(spread, spread)
    by_genome = np.zeros((G + 1, G), np.int64)
    np.add.at(by_genome, (inc_spread, genomes), 1)
    cls = {"genome_genes": np.ones(len(keys), bool), "genome_core": inc_spread == G, "genome_unique": inc_spread == 1,
           "genome_accessory": (inc_spread != G) & (inc_spread != 1)}
    out = dict(label=label, size=size, spread=spread, genome_off=np.append(first, len(keys)), genomes=genomes, copies=copies,
               size_hist=np.bincount(size), spread_hist=np.bincount(spread, minlength=G + 1), spread_by_genome=by_genome)
    out.update({n: np.bincount(genomes[m], weights=copies[m], minlength=G) for n, m in cls.items()})
    out = {n: np.asarray(v).astype(np.uint32) for n, v in out.items()}
    out.update(n_sequences=len(fam), n_genomes=G, families=len(label), incidences=len(keys), max_size=int(size.max()),
               core=int((spread == G).sum()), single_copy_core=int(((spread == G) & (size == G)).sum()), unique=int((spread == 1).sum()),
               accessory=int(((spread != G) & (spread != 1)).sum()))
    return out


def curves_sets(profile: dict, orders) -> dict:
    """pan and core of every order and prefix with sets of genomes."""
    off, gen = profile["genome_off"].tolist(), profile["genomes"].tolist()
    rows = [set(gen[off[f]:off[f + 1]]) for f in range(int(profile["families"]))]
    pan, core = [], []
    for order in np.asarray(orders).tolist():
        taken, p, c = set(), [], []
        for g in order:
            taken.add(g)
            p.append(sum(1 for r in rows if r & taken))
            c.append(sum(1 for r in rows if taken <= r))
        pan.append(p); core.append(c)
    return {"pan": np.array(pan, np.uint32), "core": np.array(core, np.uint32)}


def curves_numpy(profile: dict, orders, chunk: int = 1 << 24) -> dict:
    """... with the presence matrix gathered in every order and accumulated along it."""
    F, G = int(profile["families"]), int(profile["n_genomes"])
    present = np.zeros((F, G), bool)
    present[np.repeat(np.arange(F), np.diff(profile["genome_off"].astype(np.int64))), profile["genomes"]] = True
    orders = np.asarray(orders, np.int64)
    pan, core = np.empty(orders.shape, np.uint32), np.empty(orders.shape, np.uint32)
    step = max(1, chunk // (F * G))
    for a in range(0, len(orders), step):
        cols = present[:, orders[a:a + step]]                       # (F, orders, G)
        pan[a:a + step] = np.logical_or.accumulate(cols, axis=2).sum(axis=0)
        core[a:a + step] = np.logical_and.accumulate(cols, axis=2).sum(axis=0)
    return {"pan": pan, "core": core}


def first_difference(got: dict, want: dict):
    """-> None, or a sentence that names the first wrong count or array element."""
    for n in COUNTS:
        if int(got[n]) != int(want[n]):
            return f"{n}: {int(got[n])}, expected {int(want[n])}"
    for n in ARRAYS:
        a, b = np.asarray(got[n]), np.asarray(want[n])
        if a.shape != b.shape:
            return f"{n}: shape {a.shape}, expected {b.shape}"
        bad = np.argwhere(a != b)
        if len(bad):
            at = tuple(bad[0].tolist())
            return f"{n}{list(at)}: {int(a[at])}, expected {int(b[at])} ({len(bad)} elements differ)"
    return None


def first_curve_difference(got: dict, want: dict):
    for n in ("pan", "core"):
        a, b = np.asarray(got[n]), np.asarray(want[n])
        if a.shape != b.shape:
            return f"{n}: shape {a.shape}, expected {b.shape}"
        bad = np.argwhere(a != b)
        if len(bad):
            o, i = bad[0].tolist()
            return f"{n}[order {o}][prefix {i}]: {int(a[o, i])}, expected {int(b[o, i])} ({len(bad)} values differ)"
    return None


# ---- labellings ---------------------------------------------------------------------------------------------------------------
def relabel(family_of, seed: int, sparse: bool = False):
    """The same families under other labels: a member that need not be the smallest; ``sparse``: any free label below N, which
    need not be a member at all."""
    fam = np.asarray(family_of)
    rng = np.random.default_rng(seed)
    labs, inv = np.unique(fam, return_inverse=True)
    if sparse:
        new = rng.choice(len(fam), size=len(labs), replace=False)
    else:
        order = rng.permutation(len(fam))
        new = np.empty(len(labs), np.int64)
        new[inv[order]] = order                                      # the last member the shuffle reaches
    return new[inv].astype(np.uint32)


def random_labelling(seed: int, genes: int = 20000, genomes: int = 24):
    """About ``genes`` genes: planted families whose sizes fall off fast, some with copies inside a genome, the rest alone."""
    rng = np.random.default_rng(seed)
    fam, gen = [], []
    while len(fam) < genes:
        lab = len(fam)
        kind = rng.random()
        spread = genomes if kind < 0.25 else 1 if kind < 0.5 else int(rng.integers(1, genomes + 1))
        for g in rng.choice(genomes, size=spread, replace=False).tolist():
            for _ in range(1 + int(rng.random() < 0.1) * int(rng.integers(1, 4))):
                fam.append(lab); gen.append(g)
    fam, gen = np.array(fam, np.uint32), np.array(gen, np.uint32)
    order = rng.permutation(len(fam))                                # genes of a family lie anywhere
    inv = np.empty_like(order); inv[order] = np.arange(len(order))
    return inv[fam[order]].astype(np.uint32), gen[order], genomes    # (a family's label: where its first planted gene went)


def one_big_family(size: int, genomes: int, inside_one_genome: bool):
    """A family of ``size`` genes among singletons and pairs: its genes dealt over all genomes, or all of them copies inside
    genome 1 (one run of ``size`` equal keys, which crosses the tiles of sort and scan)."""
    n = size + 300
    fam = np.arange(n, dtype=np.uint32)
    gen = (np.arange(n, dtype=np.uint32) * 7 + 3) % genomes
    big = np.arange(100, 100 + size)
    fam[big] = 150                                                   # (a member that is not the smallest)
    gen[big] = 1 % genomes if inside_one_genome else np.arange(size) % genomes
    fam[[20, 40]] = 40
    return fam, gen, genomes


def spread_labelling(G: int, families: int, seed: int, core: str = "some"):
    """``families`` families over G genomes, one gene per genome each.  core = "all": every family in every genome; "none": no
    family in all of them (needs G >= 2); "some": a mix with unique, core and in-between families."""
    rng = np.random.default_rng(seed)
    fam, gen = [], []
    for f in range(families):
        if core == "all":
            spread = G
        elif core == "none":
            spread = int(rng.integers(1, G))
        else:
            spread = (1, G, max(1, G - 1), int(rng.integers(1, G + 1)))[f % 4]
        for g in rng.choice(G, size=spread, replace=False).tolist():
            fam.append(f); gen.append(g)
    fam = np.array(fam, np.int64)
    first = np.r_[0, np.flatnonzero(np.diff(fam)) + 1]
    return first[fam].astype(np.uint32), np.array(gen, np.uint32), G   # label = the family's first gene


def order_set(G: int, n: int, seed: int):
    """The identity, its reverse, then random orders: n in all."""
    rng = np.random.default_rng(seed)
    rows = [np.arange(G), np.arange(G)[::-1]] + [rng.permutation(G) for _ in range(max(0, n - 2))]
    return np.array(rows[:n], np.uint32)


@lru_cache(maxsize=None)
def profile_cases() -> dict:
    """name -> (family_of, genome_of, G)."""
    cases = {
        "one gene": (np.zeros(1, np.uint32), np.zeros(1, np.uint32), 1),
        "one gene, genome 2 of 3": (np.zeros(1, np.uint32), np.full(1, 2, np.uint32), 3),
        "all singletons": (np.arange(700, dtype=np.uint32), np.arange(700, dtype=np.uint32) % 5, 5),
        "one family holds everything": (np.full(700, 699, np.uint32), np.arange(700, dtype=np.uint32) % 5, 5),
        "a genome without a gene": (np.array([0, 0, 2, 3, 3], np.uint32), np.array([0, 3, 3, 0, 0], np.uint32), 4),
    }
    f, g, G = random_labelling(100, genes=3000, genomes=9)
    cases["labels that are not the smallest member"] = (relabel(f, 1), g, G)
    cases["sparse labels"] = (relabel(f, 2, sparse=True), g, G)
    for G in G_EDGES:
        cases[f"G = {G}"] = spread_labelling(G, 300, seed=G)
    for size in BIG_FAMILIES:
        cases[f"a family of {size} over the genomes"] = one_big_family(size, 11, False)
        cases[f"a family of {size} inside one genome"] = one_big_family(size, 11, True)
    for seed in range(4):
        cases[f"random, seed {seed}"] = random_labelling(seed)
    return cases


@lru_cache(maxsize=None)
def expected_profile(name: str) -> dict:
    f, g, G = profile_cases()[name]
    return profile_numpy(f, g, G)


@lru_cache(maxsize=None)
def curve_cases() -> dict:
    """name -> ((family_of, genome_of, G), orders)."""
    cases = {}
    for G in G_EDGES:
        cases[f"G = {G}"] = (spread_labelling(G, 150, seed=10 + G), order_set(G, 5, G))
    for n in (1, 2, 257):
        cases[f"{n} orders"] = (spread_labelling(12, 90, seed=3), order_set(12, n, n))
    for F in (PAN_TILE - 1, PAN_TILE, PAN_TILE + 1, 2 * PAN_TILE + 5):
        cases[f"{F} families"] = (spread_labelling(7, F, seed=F), order_set(7, 4, F))
    cases["every family is core"] = (spread_labelling(9, 60, seed=1, core="all"), order_set(9, 4, 1))
    cases["no family is core"] = (spread_labelling(9, 60, seed=2, core="none"), order_set(9, 4, 2))
    cases["copies and a wide family"] = (one_big_family(257, 11, False), order_set(11, 4, 3))
    cases["random labelling"] = (random_labelling(5, genes=6000, genomes=70), order_set(70, 6, 4))
    return cases


@lru_cache(maxsize=None)
def expected_curves(name: str):
    (f, g, G), orders = curve_cases()[name]
    prof = profile_numpy(f, g, G)
    return prof, curves_numpy(prof, orders)
