"""``.faa`` -> ``.clus`` with the gene network never written down: the whole of ``pandelos.sh`` after the k selection, the
components and collision flags of the network made on the device (K-fam, ``pdl_compute_families``) from the edges where the
best-hit filter left them.

    python -m pandelos_amd.families -i in.faa -k K|auto -o out.clus [--net out.net]

Only what Girvan-Newman has to split — the components that hold a collision, a handful of tiny ones where there are any —
is walked on the host (``netclu.families_from_components``), and only then do the edges come to Python at all.  The ``.clus``
is ``netclu.clus_text``'s: what ``netclu_ng.py`` and the text filter of ``pandelos.sh:79`` leave, genes in no family with the
script's trailing blank.  ``--net`` also writes the ``.net`` of ``python -m pandelos_amd.pangenes``.
"""
from __future__ import annotations

import argparse
import sys
from typing import Sequence

import numpy as np

from . import netclu


def gather_edges(native, nof_genomes: int):
    """Every genome task's edges in insertion order (``pdl_compute_edges``) -> (src, dst, score)."""
    parts = [native.generate_edges_part(g) for g in range(nof_genomes)]
    if not parts:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def clus_from_native(native, names, genome_of, nof_genomes: int, want_edges: bool = False):
    """-> (text of the ``.clus``, the ``pdl_families`` dict, the edges or None when nobody needed them)."""
    fam = native.generate_families()
    edges = gather_edges(native, nof_genomes) if want_edges or fam["colliding"] else None
    src, dst = (edges[0], edges[1]) if edges is not None else (None, None)
    fams, singles = netclu.families_from_components(names, genome_of, fam, src, dst)
    return netclu.clus_text(names, fams, singles), fam, edges


def main(argv: Sequence[str] | None = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m pandelos_amd.families", description="gene families (.clus) of a .faa on the MI355X")
    ap.add_argument("-i", "--input", required=True, help="Input file (.faa) to process")
    ap.add_argument("-k", "--kvalue", required=True, help="Length of the k-mers, or `auto` (calculate_k.py's choice)")
    ap.add_argument("-o", "--output", required=True, help="Output file for the gene families (.clus)")
    ap.add_argument("--net", default=None, help="Also write the network (.net)")
    args = ap.parse_args(argv)
    from .pangene_native import PangeneNative
    nativ = PangeneNative.open()
    ing = nativ.ingest_faa(args.input)
    k = ing["k_suggested"] if args.kvalue == "auto" else int(args.kvalue)
    nativ.preprocess_ingested(k)
    names, genome_of = netclu.read_names(args.input)
    if len(names) != ing["sequences"]:
        print(f"{args.input}: {len(names)} header lines by line parity, {ing['sequences']} sequences read", file=sys.stderr)
        return 1
    text, fam, edges = clus_from_native(nativ, names, genome_of, ing["genomes"], want_edges=args.net is not None)
    with open(args.output, "w") as f:
        f.write(text)
    if args.net is not None:
        from .pangenes import net_lines
        with open(args.net, "w") as f:
            f.writelines(net_lines(*edges))
    info = nativ.last_families_info
    print(f"k = {k}: {info['sequences']} genes, {info['nodes']} nodes, {info['families']} components, {info['colliding']} with a collision; "
          f"K-fam {info['device_ms']:.3f} ms on the device -> {args.output}")
    nativ.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
