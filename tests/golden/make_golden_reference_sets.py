#!/usr/bin/env python3
"""Regenerate tests/golden/reference_sets.json: the results of the reference's own library (oracle/_ref, JVM-less harness)
on the sets of tests/test_oracle_vs_reference.py — total and per-genome costs, the hash fallback, cells per genome and the
SHA-256 of every Scores field of every genome (bit patterns, helpers.raw).  Needs oracle/_ref built.  Only results are stored."""
import hashlib
import json
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from oracle import binding as ob                                   # noqa: E402
from tests import helpers as H                                     # noqa: E402
from tests.test_oracle_vs_reference import RANDOM_SETS, THREADS_SET, WRAPPED_SETS, random_set_id, wrapped_set_id  # noqa: E402


def record(gs, k, threads=None):
    with tempfile.TemporaryDirectory() as td:
        faa = Path(td) / "in.faa"
        gs.write_faa(faa)
        kw = {} if threads is None else {"threads": threads}
        info = ob.run_harness(ob.REF_SO, faa, k, dump=Path(td) / "ref.bin", **kw)
        ref = ob.read_dump(Path(td) / "ref.bin")
        dump_sha = hashlib.sha256((Path(td) / "ref.bin").read_bytes()).hexdigest()
    blocks = ref["per_genome"]
    return {"total_cost": info["total_cost"], "hash_fallback": bool(info["hash_fallback"]), "genome_cost": [info["genome_cost"][g] for g in range(ref["genomes"])],
            "scoresCount": [int(len(b["scores"])) for b in blocks], "dump_sha256": dump_sha,
            "sha256": [{f: hashlib.sha256(H.raw(b[f]).tobytes()).hexdigest() for f in H.FIELDS} for b in blocks]}


def main():
    assert ob.have_reference(), "oracle/_ref not built"
    out = {}
    for shape, k in RANDOM_SETS:
        out[random_set_id(shape, k)] = record(H.make_gene_set(**shape), k)
    for letters, k in WRAPPED_SETS:
        out[wrapped_set_id(letters, k)] = record(H.wrapped_rank_set(letters, seed=letters * 100 + k), k)
    shape, k = THREADS_SET
    for threads in (1, 4):
        out[f"threads{threads}_" + random_set_id(shape, k)] = record(H.make_gene_set(**shape), k, threads=threads)
    (Path(__file__).resolve().parent / "reference_sets.json").write_text(json.dumps(out, indent=0) + "\n")


if __name__ == "__main__":
    main()
