"""Take genomes out of a pan-genome without a rebuild — and, with ``-a``, put others in their place.

    python -m pandelos_amd.remove -i base.faa -k K -r LABEL [-r LABEL ...] [-a new.faa ...] [--rekey] -o out.net

The base set is ingested and its dictionary built; the genomes named by their ``.faa`` labels (the header's text before the
first tab) then leave it by ``pdl_remove_genomes``: one stable compaction pass over the sorted k-mer stream in HBM, no residue
is read again.  Every ``-a`` file is appended afterwards as ``python -m pandelos_amd.append`` does (replace = remove + append in
one command).  ``out.net`` is the network of what remains: byte for byte what ``python -m pandelos_amd.pangenes`` writes for a
file that holds the remaining records (and the appended files behind them).

A label that names no genome of the base, no ``-r`` at all, or every genome named is refused before the device is touched
(exit 2).  When the library cannot prove from its keys that the remaining set has the base's alphabet (``PDL_ERR_UNSUPPORTED``:
hashed ranks, or a letter of which no k-mer is left) the command says why and rebuilds from the remaining records of the file.
With ``--rekey`` (option ``alphabet_rekey``, set before the build) the library knows the remaining alphabet exactly: a letter
that only seemed lost no longer stops it, one that is lost makes it write the keys of its stream again for the smaller
alphabet, and appended files may bring letters the set lacks.  The rebuild remains for what it still refuses (hashed ranks).
"""
from __future__ import annotations

import argparse
import sys
from typing import Sequence

import numpy as np

from .append import AppendError, check_append, print_rekey
from .pangene_idata import PangeneIData
from .pangenes import run


class RemoveError(ValueError):
    pass


def remaining_input(residues, offsets, genome_of, removed):
    """The remaining set: (residues, offsets, genome_of) of the genes whose genome is not in ``removed`` — in their order, the
    genome ids made dense again in first-seen order.  What ``pdl_remove_genomes`` promises to equal a ``pdl_preprocess`` of."""
    res = np.asarray(residues, dtype=np.uint8)
    off = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    gen = np.asarray(genome_of, dtype=np.int64)
    keep = ~np.isin(gen, np.asarray(list(removed), dtype=np.int64))
    lens = np.diff(off)
    new_off = np.zeros(int(keep.sum()) + 1, np.uint64)
    np.cumsum(lens[keep], out=new_off[1:])
    byte_keep = np.repeat(keep, lens)
    kept = gen[keep]
    # first-seen order of the genomes that stay = ascending old id (ids were dense in first-seen order already)
    old = np.unique(kept)
    new_gen = np.searchsorted(old, kept).astype(np.uint32)
    return res[byte_keep].copy(), new_off, new_gen


def check_remove(labels: Sequence[str], genome_names: Sequence[str]) -> list:
    """-> the genome ids of ``labels``; raises RemoveError for no label, an unknown one, one given twice or all genomes named."""
    if not labels:
        raise RemoveError("no genome to remove (-r LABEL)")
    ids = []
    for lab in labels:
        if lab not in genome_names:
            raise RemoveError(f"the label '{lab}' names no genome of the set")
        g = list(genome_names).index(lab)
        if g in ids:
            raise RemoveError(f"the genome '{lab}' is named twice")
        ids.append(g)
    if len(ids) == len(genome_names):
        raise RemoveError("every genome of the set is named: nothing would remain")
    return ids


def main(argv: Sequence[str] | None = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m pandelos_amd.remove")
    ap.add_argument("-i", "--input", required=True, help="base set (.faa)")
    ap.add_argument("-k", "--kvalue", required=True, type=int, help="k-mer length")
    ap.add_argument("-r", "--remove", action="append", default=[], help="label of a genome to remove (may be given several times)")
    ap.add_argument("-a", "--append", action="append", default=[], help="new genomes (.faa), appended after the removal in the order given")
    ap.add_argument("-o", "--output", required=True, help="network of the remaining set (.net)")
    ap.add_argument("--rekey", action="store_true", help="follow a change of the alphabet by re-keying the sorted stream (option alphabet_rekey)")
    args = ap.parse_args(argv)

    # every label is checked before the device is touched
    base = PangeneIData.read_from_file(args.input)
    try:
        ids = check_remove(args.remove, base.genomeNames)
        names = [n for g, n in enumerate(base.genomeNames) if g not in ids]
        new_sets = []
        for path in args.append:
            new = PangeneIData.read_from_file(path)
            check_append(new, names, path)
            names += list(new.genomeNames)
            new_sets.append(new)
    except (RemoveError, AppendError) as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    from . import _lib
    from .pangene_native import PangeneNative
    nat = PangeneNative.open()
    try:
        if args.rekey:
            nat.set_option("alphabet_rekey", 1)
        nat.ingest_faa(args.input)
        nat.preprocess_ingested(args.kvalue)
        try:
            nat.remove(ids)
            info = nat.last_remove_info
            print(f"{', '.join(args.remove)}: {info['sequences']} genes, {info['kmer_occurrences']} k-mers, {info['records']} records "
                  f"removed in {info['device_ms']:.3f} ms on the device")
            print_rekey(nat.last_rekey_info)
        except _lib.PdlError as e:
            if e.code != _lib.PDL_ERR_UNSUPPORTED:
                raise
            print(f"{e}\nrebuilding from the remaining records of {args.input}")
            nat.preprocess(args.kvalue, *remaining_input(*base.flatten(), ids))
        for path, new in zip(args.append, new_sets):
            nat.append_idata(new)
            info = nat.last_append_info
            print(f"{path}: {len(new.sequences)} genes, {len(new.genomeNames)} genome(s), {info['kmer_occurrences']} k-mers, "
                  f"{info['records']} records appended in {info['device_ms']:.3f} ms on the device")
            print_rekey(nat.last_rekey_info)
        print("------------\nCOMPUTATIONAL COSTS: ")
        print(f"Total cost: {nat.cost.total_cost} lookups")
        print(f"Linear ratio: {nat.cost.linear_ratio:g}\n------------\n")
        lines = run(nat, nat.cost.genomes)
    finally:
        nat.close()
    print(f"writing into {args.output}")
    with open(args.output, "w") as f:
        f.writelines(lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
