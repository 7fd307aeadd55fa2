"""What can be said about the gene families once they are there: the family table, the counts of ``example/quality.py`` and the
pan / core accumulation curves over random genome orders, all from one pass over a labelling on the device
(``pdl_family_profile``, ``pdl_pan_curves``).

    python -m pandelos_amd.pangenome -i in.faa (--clus in.clus | -k K|auto) [-o out.clus]
        [--quality out.txt] [--matrix out.tsv] [--curves out.tsv --orders 1000 --seed 1]
        [--shared out.tsv] [--shared-copies out.tsv] [--distance out.tsv] [--distance-copies out.tsv]

With ``--clus`` the families are read from a ``.clus``; with ``-k`` the command takes the road of ``python -m
pandelos_amd.families`` on the same context (ingest, dictionary, scores, best hits, K-fam, K-split) and profiles what comes out
(``-o`` also writes that ``.clus``).  ``--quality`` writes the stdout of the reference's ``example/quality.py`` byte for byte,
``--matrix`` the family x genome copy counts, ``--curves`` per prefix length the mean, minimum and maximum of pan, core and new
families over ``--orders`` random genome orders (numpy's ``Generator(PCG64(seed))``, made on the host: the device takes no random
numbers).  ``--shared`` and ``--shared-copies`` write the genome x genome matrices of ``pdl_genome_matrix`` (DESIGN.md section 21:
families two genomes share; the sum of the smaller copy number over the families), ``--distance`` and ``--distance-copies`` the
Jaccard distances made of them in float64.
"""
from __future__ import annotations

import argparse
import sys
from typing import Sequence

import numpy as np


def family_of_from_clus(names: Sequence[str], text: str) -> np.ndarray:
    """One label per gene from the text of a ``.clus`` (a family per line, names joined by blanks): the smallest gene id of the
    line.  A gene the file does not name carries its own id, like a gene alone on its line."""
    index = {}
    for i, n in enumerate(names):
        if n in index:
            raise ValueError(f"gene name {n!r} stands for genes {index[n]} and {i}")
        index[n] = i
    fam = np.arange(len(names), dtype=np.uint32)
    seen = np.zeros(len(names), bool)
    for line in text.splitlines():
        cols = line.strip().split(" ")
        if cols == [""]:
            continue
        try:
            ids = [index[c] for c in cols]
        except KeyError as e:
            raise ValueError(f"the .clus names {e.args[0]!r}, the .faa does not") from None
        for i in ids:
            if seen[i]:
                raise ValueError(f"gene {names[i]!r} is named twice in the .clus")
            seen[i] = True
        fam[ids] = min(ids)
    return fam


def members_by_family(profile: dict, family_of) -> list:
    """Per family of the profile (ascending label) its gene ids, ascending."""
    fam = np.asarray(family_of)
    order = np.argsort(fam, kind="stable")
    ends = np.cumsum(profile["size"])
    return [order[e - s:e] for s, e in zip(profile["size"].tolist(), ends.tolist())]


def genome_ids(genome_of: Sequence) -> tuple:
    """Genome labels of the header lines -> (dense ids in first-seen order, the labels by id)."""
    ids = {}
    gen = np.array([ids.setdefault(g, len(ids)) for g in genome_of], np.uint32)
    return gen, list(ids)


def quality_text(profile: dict, genome_names: Sequence[str], n_reads: int | None = None) -> str:
    """The stdout of the reference's ``example/quality.py dataset.faa families.clus``, byte for byte, from the profile of
    ``family_of_from_clus``'s labelling of a ``.clus`` that names every gene once.  The script's quirks are kept: row 1 of the
    first two tables is the number of genes outside multi-gene families (not a number of families), the second table counts
    multi-gene families only, genomes come in string order, and the third table leaves out the spreads that do not occur.  A set
    without any multi-gene family makes the script die on ``max()`` of nothing: ``ValueError`` here.  ``n_reads``: the script's
    "nof reads", half the line count of the ``.faa`` (the gene count of a two-line file)."""
    G, N = int(profile["n_genomes"]), int(profile["n_sequences"])
    if len(genome_names) != G or len(set(genome_names)) != G:
        raise ValueError(f"{G} distinct genome names wanted")
    size_hist, spread_hist = profile["size_hist"], profile["spread_hist"]
    if int(profile["max_size"]) < 2:
        raise ValueError("no family of two genes or more: quality.py takes the max() of an empty sequence there")
    by_name = sorted(range(G), key=lambda g: genome_names[g])
    bar, half = "-" * 40, "-" * 20
    out = [bar, f"nof genomes {G}", f"nof seqs {N}", f"nof reads {N if n_reads is None else int(n_reads)}", half, "nof seqs of each genome"]
    out += [f"{genome_names[g]} {int(profile['genome_genes'][g])}" for g in by_name]
    alone = int(size_hist[1])
    out += [bar, "cluster size distribution", "number of sequences for each gene family", half, "number of sequences\tnumber of families", f"1 {alone}"]
    out += [f"{k} {int(size_hist[k])}" for k in range(2, int(profile["max_size"]) + 1)]
    widest = max([k for k in range(2, G + 1) if spread_hist[k]], default=1)      # (of the multi-gene families: one of spread 1 is two genes of one genome)
    out += [bar, "cluster genome-spread distribution", "number of involved genomes for each gene family", half, "number of genomes\tnumber of families", f"1 {alone}"]
    out += [f"{k} {int(spread_hist[k])}" for k in range(2, widest + 1)]
    out += [bar, "per genome spread distribution", half, "number of genomes\tnumber of families", "--\t" + "".join(genome_names[g] + "\t" for g in by_name)]
    table = profile["spread_by_genome"]
    out += [f"{k}\t" + "".join(f"{int(table[k, g])}\t" for g in by_name) for k in range(G + 1) if spread_hist[k]]
    return "".join(line + "\n" for line in out)


def presence_tsv(profile: dict, family_of, names: Sequence[str], genome_names: Sequence[str]) -> str:
    """Family x genome copy counts: a header line, then per family (ascending label) the name of its first gene, its size and
    spread, one copy count per genome (by id) and its genes' names joined by blanks."""
    G = int(profile["n_genomes"])
    off, gen, cp = profile["genome_off"], profile["genomes"], profile["copies"]
    lines = ["family\tsize\tspread\t" + "\t".join(genome_names) + "\tgenes\n"]
    for f, genes in enumerate(members_by_family(profile, family_of)):
        row = np.zeros(G, np.int64)
        row[gen[off[f]:off[f + 1]]] = cp[off[f]:off[f + 1]]
        lines.append(f"{names[genes[0]]}\t{int(profile['size'][f])}\t{int(profile['spread'][f])}\t" + "\t".join(map(str, row.tolist())) + "\t"
                     + " ".join(names[g] for g in genes.tolist()) + "\n")
    return "".join(lines)


def random_orders(n_genomes: int, n_orders: int, seed: int) -> np.ndarray:
    """``n_orders`` independent uniform permutations of 0..G-1, (n_orders, G) uint32, from numpy's ``Generator(PCG64(seed))``."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.permuted(np.tile(np.arange(n_genomes, dtype=np.uint32), (n_orders, 1)), axis=1)


def presence_matrix(profile: dict) -> np.ndarray:
    """(F, G) bool: family f has a gene in genome g."""
    F, G = int(profile["families"]), int(profile["n_genomes"])
    present = np.zeros((F, G), bool)
    present[np.repeat(np.arange(F), np.diff(profile["genome_off"].astype(np.int64))), profile["genomes"]] = True
    return present


def copies_matrix(profile: dict) -> np.ndarray:
    """(F, G) int64: the genes family f has in genome g."""
    F, G = int(profile["families"]), int(profile["n_genomes"])
    copies = np.zeros((F, G), np.int64)
    copies[np.repeat(np.arange(F), np.diff(profile["genome_off"].astype(np.int64))), profile["genomes"]] = profile["copies"]
    return copies


def genome_matrix_host(profile: dict) -> dict:
    """``PangeneNative.genome_matrix`` in numpy, the tests' reference and the timing baseline, as fast as numpy makes it: per copy
    level t the plane [copies >= t] of the families that reach t, against itself as a matrix product — shared is the product of
    level 1, shared_copies the sum over the levels (min(a, b) = the levels both reach).  The products run in float64 through the
    BLAS numpy is linked with (an integer ``@`` has no such road and takes a hundred times as long); every entry is a sum of
    ones and stays far below 2^53, so the integers are exact."""
    copies = copies_matrix(profile)
    most = copies.max(axis=1)
    G = copies.shape[1]
    shared, shared_copies = None, np.zeros((G, G), np.float64)
    for t in range(1, int(most.max()) + 1):
        plane = (copies[most >= t] >= t).astype(np.float64)
        product = plane.T @ plane
        shared = product if t == 1 else shared
        shared_copies += product
    return {"shared": shared.astype(np.uint32), "shared_copies": shared_copies.astype(np.uint32)}


def jaccard_distance(m) -> np.ndarray:
    """Gene-content distance from either matrix of ``genome_matrix``: 1 - m[g, h] / (m[g, g] + m[h, h] - m[g, h]) in float64
    from the exact integers, 0.0 where the union is 0 (two genomes without a gene)."""
    m = np.asarray(m).astype(np.int64)
    d = np.diag(m)
    union = d[:, None] + d[None, :] - m
    out = np.zeros(m.shape, np.float64)
    np.divide(m, union, out=out, where=union != 0)
    return np.where(union != 0, 1.0 - out, 0.0)


def pair_pan_core(shared) -> tuple:
    """Pan and core of every pair of genomes from ``shared``: pan2[g, h] = s[g, g] + s[h, h] - s[g, h] families in g or h,
    core2[g, h] = s[g, h] in both (int64)."""
    s = np.asarray(shared).astype(np.int64)
    d = np.diag(s)
    return d[:, None] + d[None, :] - s, s.copy()


def matrix_tsv(m, genome_names: Sequence[str]) -> str:
    """A square table: a header row and a first column of genome names; integers as integers, floats by ``repr``."""
    m = np.asarray(m)
    if m.ndim != 2 or m.shape != (len(genome_names), len(genome_names)):
        raise ValueError(f"a ({len(genome_names)}, {len(genome_names)}) matrix wanted")
    cell = repr if m.dtype.kind == "f" else str
    lines = ["\t" + "\t".join(genome_names) + "\n"]
    lines += [name + "\t" + "\t".join(cell(v) for v in row) + "\n" for name, row in zip(genome_names, m.tolist())]
    return "".join(lines)


def pan_curves_host(profile: dict, orders) -> dict:
    """``PangeneNative.pan_curves`` in numpy, the tests' reference and the timing baseline: per order the presence matrix with its
    columns in that order, every family's first present and first absent column, and the running counts of both."""
    orders = np.asarray(orders, dtype=np.int64)
    F, G = int(profile["families"]), int(profile["n_genomes"])
    present = presence_matrix(profile).view(np.uint8)
    pan, core = np.empty(orders.shape, np.uint32), np.empty(orders.shape, np.uint32)
    for o, order in enumerate(orders):
        cols = present[:, order]
        first = cols.argmax(axis=1)                                   # (every family has a genome)
        run = np.where(cols.all(axis=1), G, cols.argmin(axis=1))      # leading columns that hold the family
        pan[o] = np.cumsum(np.bincount(first, minlength=G))
        core[o] = F - np.cumsum(np.bincount(run, minlength=G + 1)[:G])
    return {"pan": pan, "core": core}


def curves_tsv(curves: dict) -> str:
    """Per prefix length (genomes taken in) the mean, minimum and maximum over the orders of pan, core and new (the families the
    last genome of the prefix brought: pan's step)."""
    pan, core = curves["pan"].astype(np.int64), curves["core"].astype(np.int64)
    new = np.diff(pan, axis=1, prepend=0)
    lines = ["genomes\t" + "\t".join(f"{n}_{s}" for n in ("pan", "core", "new") for s in ("mean", "min", "max")) + "\n"]
    for i in range(pan.shape[1]):
        lines.append(f"{i + 1}\t" + "\t".join(f"{a[:, i].mean():.3f}\t{a[:, i].min()}\t{a[:, i].max()}" for a in (pan, core, new)) + "\n")
    return "".join(lines)


def main(argv: Sequence[str] | None = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m pandelos_amd.pangenome", description="pan-genome profile of the gene families of a .faa on the MI355X")
    ap.add_argument("-i", "--input", required=True, help="Input file (.faa)")
    ap.add_argument("--clus", default=None, help="Gene families (.clus) of the input")
    ap.add_argument("-k", "--kvalue", default=None, help="Without --clus: make the families, with k-mers of this length, or `auto`")
    ap.add_argument("-o", "--output", default=None, help="With -k: also write the gene families (.clus)")
    ap.add_argument("--quality", default=None, help="Write the text of the reference's example/quality.py")
    ap.add_argument("--matrix", default=None, help="Write the family x genome copy counts (.tsv)")
    ap.add_argument("--curves", default=None, help="Write the pan / core accumulation curves (.tsv)")
    ap.add_argument("--orders", type=int, default=1000, help="Random genome orders of the curves")
    ap.add_argument("--seed", type=int, default=1, help="Seed of the orders")
    ap.add_argument("--shared", default=None, help="Write the genome x genome matrix of shared families (.tsv)")
    ap.add_argument("--shared-copies", default=None, help="Write the genome x genome matrix of shared gene copies, the sum of min(copies) over the families (.tsv)")
    ap.add_argument("--distance", default=None, help="Write the Jaccard distance of the genomes' family sets (.tsv)")
    ap.add_argument("--distance-copies", default=None, help="Write the multiset Jaccard distance over the families' copy numbers (.tsv)")
    args = ap.parse_args(argv)
    if (args.clus is None) == (args.kvalue is None):
        ap.error("one of --clus and -k/--kvalue")
    from . import netclu
    from .pangene_native import PangeneNative
    names, genome_of = netclu.read_names(args.input)
    with open(args.input, "rb") as f:
        n_reads = sum(1 for _ in f) // 2
    nativ = PangeneNative.open()
    if args.clus is not None:
        with open(args.clus, "r") as f:
            text = f.read()
    else:
        from . import families as FAM
        ing = nativ.ingest_faa(args.input)
        k = ing["k_suggested"] if args.kvalue == "auto" else int(args.kvalue)
        nativ.preprocess_ingested(k)
        if len(names) != ing["sequences"]:
            print(f"{args.input}: {len(names)} header lines by line parity, {ing['sequences']} sequences read", file=sys.stderr)
            return 1
        text, _, _ = FAM.clus_from_native(nativ, names, genome_of, ing["genomes"], first_level=FAM.DeviceSplitter(nativ))
        if args.output is not None:
            with open(args.output, "w") as f:
                f.write(text)
    family_of = family_of_from_clus(names, text)
    gen, genome_names = genome_ids(genome_of)
    prof = nativ.family_profile(family_of, gen, len(genome_names))
    info = nativ.last_profile_info
    print(f"{prof['n_sequences']} genes in {prof['n_genomes']} genomes: {prof['families']} families, {prof['core']} core "
          f"({prof['single_copy_core']} single-copy), {prof['accessory']} accessory, {prof['unique']} unique; "
          f"profile {info['device_ms']:.3f} ms on the device")
    if args.quality is not None:
        with open(args.quality, "w") as f:
            f.write(quality_text(prof, genome_names, n_reads))
    if args.matrix is not None:
        with open(args.matrix, "w") as f:
            f.write(presence_tsv(prof, family_of, names, genome_names))
    if args.curves is not None:
        curves = nativ.pan_curves(prof, random_orders(prof["n_genomes"], args.orders, args.seed))
        with open(args.curves, "w") as f:
            f.write(curves_tsv(curves))
        print(f"{args.orders} orders: pan and core curves in {nativ.last_curves_info['device_ms']:.3f} ms on the device -> {args.curves}")
    wanted = [(args.shared, "shared", False), (args.shared_copies, "shared_copies", False), (args.distance, "shared", True),
              (args.distance_copies, "shared_copies", True)]
    if any(path is not None for path, _, _ in wanted):
        mats = nativ.genome_matrix(prof)
        for path, which, distance in wanted:
            if path is not None:
                with open(path, "w") as f:
                    f.write(matrix_tsv(jaccard_distance(mats[which]) if distance else mats[which], genome_names))
        print(f"{prof['n_genomes']} x {prof['n_genomes']} genomes: shared families and copies over {mats['levels']} bit columns in "
              f"{mats['device_ms']:.3f} ms on the device")
    nativ.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
