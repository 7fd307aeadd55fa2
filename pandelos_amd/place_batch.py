"""Place many newly sequenced genomes into a pan-genome's gene families in one pass, each on its own, without a commit.

    python -m pandelos_amd.place_batch -i base.faa -k K -q new.faa [-q more.faa ...] --out-dir DIR [--net] [--rekey]

The base set is ingested, its dictionary built and its families clustered once on the device; every genome of the query files,
in first-seen order, is an independent query of ``pdl_place_batch``: its placement is the one ``python -m pandelos_amd.place``
gets for that genome alone.  The queries never see each other — two that touch the same base family each get that family and
do not fuse; genomes that should be clustered with each other are appended (``python -m pandelos_amd.append``).

``DIR/<label>.tsv`` holds one line per gene of the genome (the columns of ``pandelos_amd.place``) and, with ``--net``,
``DIR/<label>.net`` the edges the genome's own task adds to the network; both byte for byte what ``pandelos_amd.place`` writes
for that genome.

Refused before the device is touched, as by ``pandelos_amd.query_batch``: a label that already names a base genome, a label
seen in two query files, and a label that is not a safe file name.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Sequence

from .pangene_idata import PangeneIData
from .pangenes import net_lines
from .place import placement_rows, tsv_text
from .query import QueryError
from .query_batch import collect_queries


def main(argv: Sequence[str] | None = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m pandelos_amd.place_batch")
    ap.add_argument("-i", "--input", required=True, help="base set (.faa)")
    ap.add_argument("-k", "--kvalue", required=True, type=int, help="k-mer length (that of the base run)")
    ap.add_argument("-q", "--query", required=True, action="append", help="new genomes (.faa, one or more genomes); may be given several times")
    ap.add_argument("--out-dir", required=True, help="directory of the <label>.tsv (and <label>.net) files")
    ap.add_argument("--net", action="store_true", help="also write the edges of each genome's task (<label>.net)")
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
        pls = nat.place_batch_idata([d for _, d in queries])
        info = nat.last_place_batch_info
    finally:
        nat.close()
    os.makedirs(args.out_dir, exist_ok=True)
    for (label, data), pl, pi in zip(queries, pls, info["queries"]):
        tsv = os.path.join(args.out_dir, label + ".tsv")
        with open(tsv, "w") as f:
            f.write(tsv_text(placement_rows(pl, list(base.sequenceName) + list(data.sequenceName))))
        if args.net:
            with open(os.path.join(args.out_dir, label + ".net"), "w") as f:
                f.writelines(net_lines(pl["src"], pl["dst"], pl["score"]))
        print(f"query genome '{label}': {len(data.sequences)} genes against {ing['sequences']} base genes; {pi['edges']} edges; "
              f"{pl['groups']} families touched: {pl['novel']} novel, {pl['joined']} joined, {pl['bridging']} bridging, {pl['colliding']} colliding; "
              f"{pl['unplaced']} genes unplaced -> {tsv}")
    print(f"{len(queries)} queries in {info['chunks']} chunk(s), {info['device_ms']:.3f} ms on the device")
    return 0


if __name__ == "__main__":
    sys.exit(main())
