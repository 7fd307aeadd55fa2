"""``.faa`` -> ``.clus`` with the gene network never written down: the whole of ``pandelos.sh`` after the k selection, the
components and collision flags of the network made on the device (K-fam, ``pdl_compute_families``) from the edges where the
best-hit filter left them.

    python -m pandelos_amd.families -i in.faa -k K|auto -o out.clus [--net out.net] [--host-split]
    python -m pandelos_amd.families -i in.faa --from-net in.net -o out.clus [--host-split]

Only what Girvan-Newman has to split — the components that hold a collision — comes to Python at all: the host keeps the
orders (``netclu.split_all_until_clean``), the device removes the edges (K-split, ``pdl_split_first_level``: every component
pending at one level of the recursion in one call).  ``--host-split`` keeps the whole split on the host
(``netclu.split_until_clean``); the ``.clus`` bytes are the same either way.  ``--from-net`` takes the network from a ``.net``
instead of scoring the ``.faa`` (only its header lines are read then, and ``-k`` is not needed): K-fam over the file's edges
(``pdl_families_of_edges``), then the same split.  The ``.clus``
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


class DeviceSplitter:
    """The splitter ``netclu.split_all_until_clean`` takes, on the device (``PangeneNative.split_first_level``): all graphs of a
    level in one call, whatever their size (the device road wins on components of 16 genes too).
    ``totals`` adds up the calls' ``last_split_info``."""

    def __init__(self, native):
        self.native = native
        self.totals = {"calls": 0, "graphs": 0, "nodes": 0, "edges": 0, "removals": 0, "rounds": 0, "chunks": 0, "device_ms": 0.0}

    def __call__(self, graphs):
        out = self.native.split_first_level(graphs)
        self.totals["calls"] += 1
        for key, val in self.native.last_split_info.items():
            self.totals[key] += val
        return out


last_split_info = None     # what the last run of the command (``main``) left: the last call's ``last_split_info`` and the run's totals


def clus_from_native(native, names, genome_of, nof_genomes: int, want_edges: bool = False, first_level=None):
    """-> (text of the ``.clus``, the ``pdl_families`` dict, the edges or None when nobody needed them).  ``first_level``: the
    splitter of the colliding components (a ``DeviceSplitter``); None: the host's recursion."""
    fam = native.generate_families()
    edges = gather_edges(native, nof_genomes) if want_edges or fam["colliding"] else None
    src, dst = (edges[0], edges[1]) if edges is not None else (None, None)
    fams, singles = netclu.families_from_components(names, genome_of, fam, src, dst, first_level=first_level)
    return netclu.clus_text(names, fams, singles), fam, edges


def _report_split(nativ, splitter) -> None:
    """Closes a run of the command: ``families.last_split_info`` (None with ``--host-split``, or when nothing collided), and a line."""
    global last_split_info
    last_split_info = None
    if splitter is not None and splitter.totals["calls"]:
        t = splitter.totals
        last_split_info = dict(nativ.last_split_info, totals=dict(t))
        print(f"K-split: {t['graphs']} graphs in {t['calls']} calls, {t['removals']} edges removed, {t['device_ms']:.3f} ms on the device")


def _from_net(nativ, args) -> int:
    """``--from-net``: K-fam over the edges of a ``.net`` (``pdl_families_of_edges``), then the split — ``netclu``'s road with the
    components and the removals made on the device."""
    names, genome_of = netclu.read_names(args.input)
    src, dst = netclu.read_net_edges(args.from_net)
    ids = {}
    gen = np.array([ids.setdefault(g, len(ids)) for g in genome_of], np.uint32)
    fam = nativ.families_of_edges(src, dst, gen)
    splitter = None if args.host_split else DeviceSplitter(nativ)
    fams, singles = netclu.families_from_components(names, genome_of, fam, src, dst, net_ordered=True, first_level=splitter)
    with open(args.output, "w") as f:
        f.write(netclu.clus_text(names, fams, singles))
    print(f"{args.from_net}: {fam['sequences']} genes, {fam['nodes']} nodes, {fam['families']} components, {fam['colliding']} with a collision"
          f" -> {args.output}")
    _report_split(nativ, splitter)
    nativ.close()
    return 0


def main(argv: Sequence[str] | None = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m pandelos_amd.families", description="gene families (.clus) of a .faa on the MI355X")
    ap.add_argument("-i", "--input", required=True, help="Input file (.faa) to process")
    ap.add_argument("-k", "--kvalue", default=None, help="Length of the k-mers, or `auto` (calculate_k.py's choice); not needed with --from-net")
    ap.add_argument("-o", "--output", required=True, help="Output file for the gene families (.clus)")
    ap.add_argument("--net", default=None, help="Also write the network (.net)")
    ap.add_argument("--host-split", action="store_true", help="Split the colliding components on the host (netclu.split_until_clean)")
    ap.add_argument("--from-net", default=None, help="Take the network from this .net instead of scoring the .faa (its headers are still read)")
    args = ap.parse_args(argv)
    if args.kvalue is None and args.from_net is None:
        ap.error("the following arguments are required: -k/--kvalue")
    from .pangene_native import PangeneNative
    nativ = PangeneNative.open()
    if args.from_net is not None:
        return _from_net(nativ, args)
    ing = nativ.ingest_faa(args.input)
    k = ing["k_suggested"] if args.kvalue == "auto" else int(args.kvalue)
    nativ.preprocess_ingested(k)
    names, genome_of = netclu.read_names(args.input)
    if len(names) != ing["sequences"]:
        print(f"{args.input}: {len(names)} header lines by line parity, {ing['sequences']} sequences read", file=sys.stderr)
        return 1
    splitter = None if args.host_split else DeviceSplitter(nativ)
    text, fam, edges = clus_from_native(nativ, names, genome_of, ing["genomes"], want_edges=args.net is not None, first_level=splitter)
    with open(args.output, "w") as f:
        f.write(text)
    if args.net is not None:
        from .pangenes import net_lines
        with open(args.net, "w") as f:
            f.writelines(net_lines(*edges))
    info = nativ.last_families_info
    print(f"k = {k}: {info['sequences']} genes, {info['nodes']} nodes, {info['families']} components, {info['colliding']} with a collision; "
          f"K-fam {info['device_ms']:.3f} ms on the device -> {args.output}")
    _report_split(nativ, splitter)
    nativ.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
