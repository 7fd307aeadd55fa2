"""Score one newly sequenced genome against a pan-genome's dictionary without a rebuild.

    python -m pandelos_amd.query -i base.faa -k K -q new.faa -o new.net [--cells new.tsv] [--rekey]

The base set is ingested and its dictionary built once (``pdl_ingest_faa`` + ``pdl_preprocess_ingested``); the query file
(one genome, read like ``PangeneIData.readFromFile``) is scored against it with ``pdl_query_scores``: the Scores block the
reference's ``computeScores(G)`` returns for the union run (base genes first, the query genes as genome G, ids N..).

``new.net`` holds the edges the new genome's OWN task adds to the network (``bbh_edges`` + ``net_lines`` of
``pandelos_amd.pangenes`` on that block), ids in union numbering.  The edges the other genomes' tasks would add toward the
new genome are not part of it: their per-genome and per-column maxima change only in a full run of the union.

``--cells`` writes every emitted cell as ``query_gene  target_gene  target_genome  score  perc  tr_perc`` (tab-separated,
gene and genome names from the headers).

A residue the base set lacks (one ``X``, ``U``, ``B``, ``Z`` or ``*``) is refused, since the union would rank k-mers differently;
``--rekey`` (option ``query_rekey``) ranks the query in the union's alphabet instead and returns the union run's block.

A query file that holds more than one genome (or none), or a genome whose label already names a base genome, is refused:
in the union the genes of such a label would join that genome.
"""
from __future__ import annotations

import argparse
import sys
from typing import Sequence

import numpy as np

from .pangene_idata import PangeneIData
from .pangenes import bbh_edges, net_lines


class QueryError(ValueError):
    pass


def check_query(query: PangeneIData, base_genome_names: Sequence[str]) -> None:
    if len(query.genomeNames) != 1:
        raise QueryError(f"the query file must hold exactly one genome, it holds {len(query.genomeNames)}")
    if query.genomeNames[0] in set(base_genome_names):
        raise QueryError(f"the query genome '{query.genomeNames[0]}' already names a base genome: its genes would join it")


def write_outputs(block, base: PangeneIData, query: PangeneIData, net_path, cells_path=None) -> int:
    """The `.net` of one query block and, with ``cells_path``, its cells with names; -> edges written."""
    src, dst, score = bbh_edges(block)
    with open(net_path, "w") as f:
        f.writelines(net_lines(src, dst, score))
    if cells_path:
        names = list(base.sequenceName) + list(query.sequenceName)
        genomes = list(base.genomeNames) + [query.genomeNames[0]]
        with open(cells_path, "w") as f:
            for r, c, g2, s, p, t in zip(block.row.tolist(), block.column.tolist(), block.second_seq_genome.tolist(),
                                         block.scores.astype(np.float64).tolist(), block.percs.astype(np.float64).tolist(),
                                         block.tr_percs.astype(np.float64).tolist()):
                f.write(f"{names[r]}\t{names[c]}\t{genomes[g2]}\t{s!r}\t{p!r}\t{t!r}\n")
    return len(src)


def main(argv: Sequence[str] | None = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m pandelos_amd.query")
    ap.add_argument("-i", "--input", required=True, help="base set (.faa)")
    ap.add_argument("-k", "--kvalue", required=True, type=int, help="k-mer length (that of the base run)")
    ap.add_argument("-q", "--query", required=True, help="the new genome (.faa, one genome)")
    ap.add_argument("-o", "--output", required=True, help="edges of the new genome's task (.net)")
    ap.add_argument("--cells", default=None, help="every emitted cell of the new genome, with names (.tsv)")
    ap.add_argument("--rekey", action="store_true", help="accept letters the base lacks: rank the query in the union's alphabet (option query_rekey)")
    args = ap.parse_args(argv)

    base = PangeneIData.read_from_file(args.input)          # (names for --cells and the label check)
    query = PangeneIData.read_from_file(args.query)
    try:
        check_query(query, base.genomeNames)
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
        block = nat.query_idata(query)
        info = nat.last_query_info
    finally:
        nat.close()
    n_edges = write_outputs(block, base, query, args.output, args.cells)
    print(f"query genome '{query.genomeNames[0]}': {len(query.sequences)} genes against {ing['sequences']} base genes; "
          f"Genome {ing['genomes']} cost = {info['genome_cost']}; {block.scoresCount} cells, {n_edges} edges -> {args.output}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
