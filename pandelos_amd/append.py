"""Grow a pan-genome a file at a time: build the base set's dictionary once, append newly sequenced genomes by a merge.

    python -m pandelos_amd.append -i base.faa -k K -a new1.faa [-a new2.faa ...] [--rekey] -o union.net

The base set is ingested and its dictionary built (``pdl_ingest_faa`` + ``pdl_preprocess_ingested``); every ``-a`` file (read
like ``PangeneIData.readFromFile``; it may hold several genomes) is then appended in turn with ``pdl_append_genomes``: its
k-mers are ranked and sorted alone and merged into the sorted stream in HBM, the base's residues are not read again.  The
context afterwards is the one a build on the concatenated files would leave, and ``union.net`` is the network of that
union (``pandelos_amd.pangenes.run``): byte for byte what ``python -m pandelos_amd.pangenes`` writes for the concatenation.

A genome label in an appended file that already names a genome of the context (of the base or of an earlier ``-a`` file) is
refused (exit 2): in the union its genes would join that genome, which an append cannot do.

A letter in an appended file that the set so far lacks changes the rank of every k-mer: the library refuses it, unless
``--rekey`` (option ``alphabet_rekey``) lets it write the keys of its sorted stream again for the union's alphabet — one more
streaming pass, still no residue of the base read.
"""
from __future__ import annotations

import argparse
import sys
from typing import Sequence

from .pangene_idata import PangeneIData
from .pangenes import run


class AppendError(ValueError):
    pass


def check_append(new: PangeneIData, genome_names: Sequence[str], path: str = "") -> None:
    """Raises AppendError when the file holds no gene or one of its genome labels already names a genome of the context."""
    where = f"{path}: " if path else ""
    if not new.sequences:
        raise AppendError(f"{where}the file holds no gene")
    known = set(genome_names)
    for name in new.genomeNames:
        if name in known:
            raise AppendError(f"{where}the genome '{name}' already names a genome of the set: its genes would join it")


def print_rekey(rk: dict) -> None:
    """One line about a call that changed the alphabet (``PangeneNative.last_rekey_info``); nothing otherwise."""
    if rk["rekeyed"]:
        print(f"  alphabet {rk['letters_before']} -> {rk['letters_after']} letters, keys {rk['key_bits_before']} -> {rk['key_bits_after']} bits: "
              f"{rk['keys_rewritten']} keys written again in {rk['rekey_ms']:.3f} ms")


def main(argv: Sequence[str] | None = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m pandelos_amd.append")
    ap.add_argument("-i", "--input", required=True, help="base set (.faa)")
    ap.add_argument("-k", "--kvalue", required=True, type=int, help="k-mer length")
    ap.add_argument("-a", "--append", required=True, action="append", help="new genomes (.faa), appended in the order given")
    ap.add_argument("-o", "--output", required=True, help="network of the union (.net)")
    ap.add_argument("--rekey", action="store_true", help="accept letters the set lacks: re-key the sorted stream (option alphabet_rekey)")
    args = ap.parse_args(argv)

    # every label is checked before the device is touched
    names = list(PangeneIData.read_from_file(args.input).genomeNames)
    new_sets = []
    for path in args.append:
        new = PangeneIData.read_from_file(path)
        try:
            check_append(new, names, path)
        except AppendError as e:
            print(f"error: {e}", file=sys.stderr)
            return 2
        names += list(new.genomeNames)
        new_sets.append(new)
    from .pangene_native import PangeneNative
    nat = PangeneNative.open()
    try:
        if args.rekey:
            nat.set_option("alphabet_rekey", 1)
        nat.ingest_faa(args.input)
        nat.preprocess_ingested(args.kvalue)
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
