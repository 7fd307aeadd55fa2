#!/usr/bin/env python3
"""Regenerate tests/golden/query_rekey/<case>.npz — fixtures of pdl_query_scores under option "query_rekey": queries that bring
letters the base lacks — FROM THE REFERENCE ITSELF, in the shape of make_golden_query.py.

A case is a base set and a one-genome query set whose residues hold at least one byte no base gene holds.  The reference build
(oracle/_ref/libnative_ref.so through oracle/jni_harness) scores the UNION: the base genes in base order, then the query genes as
genome G.  Stored per case: base_faa, query_faa, k, G, genome_cost and genome G's Scores block (float32 as raw bit patterns).

The cases are the four shapes of the union's last-record fold (pdl_query.h, Q1) ACROSS an alphabet change, a letter that lives
only in a query gene shorter than k, and two letters at once.  `fold_shape` says from the k-mers alone which shape a case has
(ranks order k-mers as their bytes do), and the maker refuses to write a case that has another shape than its name says.

Data only (inputs and expected outputs): nothing of the reference's source is stored.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from oracle import binding as ob                                              # noqa: E402
from tests.golden.make_golden_query import FIELDS, faa_of, raw, run_union     # noqa: E402
from tests.test_rekey_cpu import family_genes, with_letters                   # noqa: E402

HERE = Path(__file__).resolve().parent
OUT = HERE / "query_rekey"


def kmer_records(genes, k):
    """{k-mer: set of genes that hold it} — the records of a dictionary, grouped by rank"""
    out = {}
    for i, g in enumerate(genes):
        for j in range(len(g) - k + 1):
            out.setdefault(g[j:j + k], set()).add(i)
    return out


def fold_shape(base_genes, query_genes, k):
    """Q1 of the union by the k-mers' bytes: 'a' the query's last record, alone in its rank, folds (into 'a:base' the base's last
    group or 'a:query' a query group); 'b' qmax == bmax; 'c' the base's lonely last record joins a query group; 'none'."""
    b, q = kmer_records(base_genes, k), kmer_records(query_genes, k)
    bmax, qmax = max(b), max(q)
    if qmax > bmax:
        if len(q[qmax]) > 1:
            return "none"
        below = [x for x in q if x < qmax]
        return "a:query" if below and max(below) > bmax else "a:base"
    if qmax == bmax:
        return "b"
    lonely = len(b[bmax]) == 1
    r2 = max((x for x in b if x < bmax), default=None)
    return "c" if lonely and (r2 is None or qmax > r2) else "none"


def family_case(alphabet, seed, k, genes=8, lo=12, hi=30):
    """three base genomes and a fourth, the query's, of one ancestor over `alphabet` -> (base [(label, gene)], query genes)"""
    fam = family_genes(alphabet, 4, genes, max(lo, k + 2), hi, seed)
    base = [(b"G%d" % g, s) for g in range(3) for s in fam[g]]
    return base, list(fam[3])


def make_cases():
    """name -> (base records, query genes, k, expected fold shape, letters the query brings)"""
    cases = {}
    # 1. the query's last record alone holds 'Z', above every base letter; every other query rank is at most the base's largest
    base, q = family_case(b"CDEFGH", 1, 3)
    base += [(b"G0", b"HHHH"), (b"G1", b"HHHC")]
    q = q[:6] + [b"ZCDE"]
    cases["fold_a_new_letter_above_folds_into_base_last_group"] = (base, q, 3, "a:base", b"Z")
    # 2. the query holds the base's largest k-mer; the new letter sits elsewhere, at the end of a gene that starts low
    base, q = family_case(b"CDEFGH", 2, 3)
    base += [(b"G0", b"HHHH"), (b"G2", b"GHHH")]
    q = q[:6] + [b"HHHC", b"CDEZ"]
    cases["fold_b_qmax_is_bmax_new_letter_elsewhere"] = (base, q, 3, "b", b"Z")
    # 3. '*' lies below every base letter: every base digit moves.  The base's last record (HHH, one gene) is alone; the query's
    #    largest k-mer HCD lies between it and the rest of the base, so that record joins a query group
    base, q = family_case(b"CDEF", 3, 3)
    base += [(b"G1", b"HHH")]
    q = [with_letters(g, b"*", 30 + i, every=7) for i, g in enumerate(q[:6])] + [b"HCD", b"DHCDE"]
    cases["fold_c_new_letter_below_base_last_joins_query_group"] = (base, q, 3, "c", b"*")
    # 4. nothing folds: the base's largest k-mer is in two genes and above the query's; the new letter lies between base letters
    base, q = family_case(b"CDEFH", 4, 4)
    base += [(b"G0", b"HHHHC"), (b"G2", b"DHHHH")]
    q = [with_letters(g, b"G", 40 + i, every=8) for i, g in enumerate(q[:7])]
    cases["fold_none_new_letter_between"] = (base, q, 4, "none", b"G")
    # a letter that lives only in a query gene shorter than k: it shows in no key and still changes every rank
    base, q = family_case(b"DEFGHIK", 5, 4)
    q = q[:7] + [b"AAA", b"A"]
    cases["new_letter_only_in_a_short_gene"] = (base, q, 4, None, b"A")
    # two letters at once, one of them between base letters
    base, q = family_case(b"CDEFHIK", 6, 3)
    q = [with_letters(g, b"GX", 60 + i, every=6) for i, g in enumerate(q)]
    cases["two_letters_one_between"] = (base, q, 3, None, b"GX")
    return cases


def main():
    assert ob.have_reference(), "build oracle/_ref first (python __graft_entry__.py)"
    OUT.mkdir(exist_ok=True)
    only = set(sys.argv[1:])
    for name, (base, q, k, shape, letters) in make_cases().items():
        if only and name not in only:
            continue
        base_letters = set(b"".join(s for _, s in base))
        assert set(b"".join(q)) - base_letters == set(letters), (name, set(b"".join(q)) - base_letters)
        if shape is not None:
            assert fold_shape([s for _, s in base], q, k) == shape, (name, fold_shape([s for _, s in base], q, k))
        base_faa, query_faa = faa_of(base, b"b"), faa_of([(b"Q", s) for s in q], b"q")
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
