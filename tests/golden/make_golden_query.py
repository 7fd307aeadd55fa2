#!/usr/bin/env python3
"""Regenerate tests/golden/query/<case>.npz — fixtures of pdl_query_scores — FROM THE REFERENCE ITSELF.

A case is a base set and a one-genome query set.  The reference build (oracle/_ref/libnative_ref.so through
oracle/jni_harness, as make_golden.py runs it) scores the UNION: the base genes in base order, then the query genes as
genome G.  Stored per case:

  base_faa, query_faa   input bytes (the union file is base_faa + query_faa)
  k, G                  k-mer length, id of the query genome in the union
  genome_cost           "Genome G cost" printed by the reference
  <field>               genome G's Scores block (float32 kept as raw bit patterns)

Data only (inputs and expected outputs): nothing of the reference's source is stored.
"""
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from oracle import binding as ob                      # noqa: E402
from pandelos_amd.synth import make_gene_set          # noqa: E402

HERE = Path(__file__).resolve().parent
OUT = HERE / "query"
FIELDS = ("scores", "percs", "tr_percs", "row", "column", "first_seq_genome", "second_seq_genome",
          "max_genome_score", "max_genome_score_col", "scoresMaxMappings")


def faa_of(recs, tag=b"g"):
    return b"".join(b"%s\t%s%d\tprod\n%s\n" % (g, tag, i, s) for i, (g, s) in enumerate(recs))


def held_out(genomes, genes_per_genome, mean_len, seed, protein_like=False, sub_rate=0.1):
    """A synthetic set split into (base faa, query faa): the query is its last genome."""
    gs = make_gene_set(genomes=genomes, genes_per_genome=genes_per_genome, mean_len=mean_len, sub_rate=sub_rate, seed=seed,
                       protein_like=protein_like)
    last = int(gs.genome_of.max())
    base, query = [], []
    for i in range(len(gs.genome_of)):
        s = gs.residues[int(gs.offsets[i]):int(gs.offsets[i + 1])].tobytes()
        g = int(gs.genome_of[i])
        (query if g == last else base).append((b"G%d" % g, s))
    return faa_of(base, b"b"), faa_of(query, b"q")


def wide_row():
    """One low-complexity query gene that shares its only k-mer with 9000 base genes: a row of 9000 distinct columns."""
    rng = np.random.default_rng(5)
    letters = np.frombuffer(b"ACDEFGHIKL", np.uint8)
    base = []
    for i in range(9000):
        tail = letters[rng.integers(0, len(letters), 3)].tobytes()
        base.append((b"B%d" % (i % 3), b"AAA" + tail))
    base.append((b"B0", b"ACDEFGHIKL"))
    return faa_of(base, b"b"), faa_of([(b"Q", b"AAAA"), (b"Q", b"CDEFAAA")], b"q"), 3


CASES = {   # name -> (base faa, query faa, k)
    # Q1 of the union: (a) a query k-mer above the base maximum, in one query gene, folded into a base group
    "q1a_query_max_folds_into_base_group": (faa_of([(b"a", b"AAC"), (b"b", b"ACA"), (b"c", b"CACAG")]),
                                            faa_of([(b"x", b"AGG"), (b"x", b"AAC")], b"q"), 2),
    # (b) the base's folded last record shares its rank with a query record: the fold is undone
    "q1b_base_fold_undone": (faa_of([(b"a", b"AAC"), (b"b", b"ACA"), (b"c", b"CC")]),
                             faa_of([(b"x", b"CCA")], b"q"), 2),
    # (c) the base's last singleton stays last, the union's second-highest rank is a query rank
    "q1c_base_last_folds_into_query_group": (faa_of([(b"a", b"AAC"), (b"b", b"ACA"), (b"c", b"CG")]),
                                             faa_of([(b"x", b"ACC"), (b"x", b"CCA")], b"q"), 2),
    # (d) the query holds the base maximum, whose group already has two records
    "q1d_query_joins_base_max_group": (faa_of([(b"a", b"AAC"), (b"b", b"ACA"), (b"c", b"CAC")]),
                                       faa_of([(b"x", b"CAA")], b"q"), 2),
    "identical_gene": (faa_of([(b"a", b"MKVLAAGIVGLLLAQ"), (b"b", b"MKVLAAGIVGLLLSQ"), (b"b", b"PPQRSTWYAC")]),
                       faa_of([(b"x", b"MKVLAAGIVGLLLAQ"), (b"x", b"WYACPPQ")], b"q"), 3),
    "short_query_genes": (faa_of([(b"a", b"ACDEFGHIK"), (b"b", b"CDEFGHIKA"), (b"c", b"AC")]),
                          faa_of([(b"x", b"AC"), (b"x", b"A"), (b"x", b"ACDEFG"), (b"x", b"CDE")], b"q"), 3),
    "repeated_kmer_in_query_gene": (faa_of([(b"a", b"ACDACDKLM"), (b"b", b"ACDKLMACD"), (b"c", b"DACDA")]),
                                    faa_of([(b"x", b"ACDACDACDACD"), (b"x", b"KLMKLM")], b"q"), 3),
    "hash_fallback_20_letters_k16": held_out(4, 30, 70, 161) + (16,),
    "two_letters": (faa_of([(b"a", b"ABBABAAB"), (b"a", b"BBBBAAAA"), (b"b", b"ABABABAB"), (b"c", b"AABBAABB")]),
                    faa_of([(b"x", b"ABBABAAB"), (b"x", b"BABA"), (b"x", b"AAAAAAAAB")], b"q"), 4),
    "protein_like_held_out": held_out(6, 40, 90, 162, protein_like=True) + (4,),
    "wide_row_9000_columns": wide_row(),
}


def run_union(base_faa, query_faa, k):
    union = base_faa + query_faa
    with tempfile.TemporaryDirectory() as td:
        p = Path(td) / "union.faa"
        p.write_bytes(union)
        info = ob.run_harness(ob.REF_SO, p, k, dump=Path(td) / "out.bin")
        return info, ob.read_dump(Path(td) / "out.bin")


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def main():
    assert ob.have_reference(), "build oracle/_ref first (python __graft_entry__.py)"
    OUT.mkdir(exist_ok=True)
    only = set(sys.argv[1:])
    for name, (base_faa, query_faa, k) in CASES.items():
        if only and name not in only:
            continue
        info, ref = run_union(base_faa, query_faa, k)
        G = ref["genomes"] - 1
        block = ref["per_genome"][G]
        out = {"base_faa": np.frombuffer(base_faa, np.uint8), "query_faa": np.frombuffer(query_faa, np.uint8),
               "k": np.int64(k), "G": np.int64(G), "genome_cost": np.uint64(info["genome_cost"][G])}
        for f in FIELDS:
            out[f] = raw(block[f])
        np.savez_compressed(OUT / f"{name}.npz", **out)
        print(name, "genes", ref["sequences"], "G", G, "cells", int(block["scoresCount"]), "cost", info["genome_cost"][G])


if __name__ == "__main__":
    main()
