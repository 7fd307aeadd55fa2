"""Score many newly sequenced genomes against a pan-genome's dictionary in one pass, each on its own.

    python -m pandelos_amd.query_batch -i base.faa -k K -q new.faa [-q more.faa ...] --out-dir DIR [--cells] [--rekey]

The base set is ingested and its dictionary built once; every genome of the query files, in first-seen order, is an
independent query of ``pdl_query_batch``: its block is the one ``python -m pandelos_amd.query`` gets for that genome alone
(``computeScores(G)`` of the union of the base and that genome only).  The queries never see each other — genomes that
should be scored against each other are appended (``python -m pandelos_amd.append``).

``DIR/<label>.net`` holds the edges the genome's own task adds to the network and, with ``--cells``, ``DIR/<label>.tsv``
every emitted cell with names; both byte for byte what ``pandelos_amd.query`` writes for that genome.

Refused before the device is touched: a label that already names a base genome (in the union its genes would join it), a
label seen in two query files (one file would overwrite the other's result), and a label that is not a safe file name.
"""
from __future__ import annotations

import argparse
import os
import re
import sys
from typing import List, Sequence, Tuple

from .pangene_idata import PangeneIData
from .query import QueryError, write_outputs

_SAFE_LABEL = re.compile(r"[A-Za-z0-9_][A-Za-z0-9._+=,@-]*\Z")


def split_genomes(data: PangeneIData) -> List[PangeneIData]:
    """One ``PangeneIData`` per genome of ``data``, in first-seen order, each with its genes in file order."""
    parts = [PangeneIData(genomeNames=[name]) for name in data.genomeNames]
    for seq, name, desc, g in zip(data.sequences, data.sequenceName, data.sequenceDescription, data.sequenceGenome):
        p = parts[g]
        p.sequences.append(seq); p.sequenceName.append(name); p.sequenceDescription.append(desc); p.sequenceGenome.append(0)
    return parts


def check_label(label: str) -> None:
    if not _SAFE_LABEL.match(label) or len(label) > 200:
        raise QueryError(f"the query genome label {label!r} is not a safe file name (letters, digits and ._+=,@- only, not starting with a dot or a dash)")


def collect_queries(files: Sequence[Tuple[str, PangeneIData]], base_genome_names: Sequence[str]) -> List[Tuple[str, PangeneIData]]:
    """``[(file name, its data)]`` -> ``[(label, one-genome data)]`` in first-seen order, or ``QueryError``."""
    base = set(base_genome_names)
    seen: dict = {}
    out = []
    for fname, data in files:
        parts = split_genomes(data)
        if not parts:
            raise QueryError(f"the query file '{fname}' holds no genome")
        for part in parts:
            label = part.genomeNames[0]
            check_label(label)
            if label in base:
                raise QueryError(f"the query genome '{label}' already names a base genome: its genes would join it")
            if label in seen:
                raise QueryError(f"the query genome '{label}' is in '{seen[label]}' and in '{fname}': each query is one genome of one file")
            seen[label] = fname
            out.append((label, part))
    return out


def main(argv: Sequence[str] | None = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m pandelos_amd.query_batch")
    ap.add_argument("-i", "--input", required=True, help="base set (.faa)")
    ap.add_argument("-k", "--kvalue", required=True, type=int, help="k-mer length (that of the base run)")
    ap.add_argument("-q", "--query", required=True, action="append", help="new genomes (.faa, one or more genomes); may be given several times")
    ap.add_argument("--out-dir", required=True, help="directory of the <label>.net (and <label>.tsv) files")
    ap.add_argument("--cells", action="store_true", help="also write every emitted cell of each genome, with names (<label>.tsv)")
    ap.add_argument("--rekey", action="store_true", help="accept letters the base lacks: rank the query in the union's alphabet (option query_rekey)")
    args = ap.parse_args(argv)

    base = PangeneIData.read_from_file(args.input)
    try:
        queries = collect_queries([(q, PangeneIData.read_from_file(q)) for q in args.query], base.genomeNames)
    except QueryError as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    from .pangene_native import PangeneNative
    nat = PangeneNative.open()
    try:
        ing = nat.ingest_faa(args.input)
        nat.preprocess_ingested(args.kvalue)
        if args.rekey:
            nat.set_option("query_rekey", 1)
        blocks = nat.query_batch_idata([d for _, d in queries])
        info = nat.last_query_batch_info
    finally:
        nat.close()
    os.makedirs(args.out_dir, exist_ok=True)
    for (label, data), block, qi in zip(queries, blocks, info["queries"]):
        net = os.path.join(args.out_dir, label + ".net")
        edges = write_outputs(block, base, data, net, os.path.join(args.out_dir, label + ".tsv") if args.cells else None)
        print(f"query genome '{label}': {len(data.sequences)} genes against {ing['sequences']} base genes; "
              f"Genome {ing['genomes']} cost = {qi['genome_cost']}; {block.scoresCount} cells, {edges} edges -> {net}")
    print(f"{len(queries)} queries in {info['chunks']} chunk(s), {info['device_ms']:.3f} ms on the device")
    return 0


if __name__ == "__main__":
    sys.exit(main())
