#!/usr/bin/env python3
"""Time the genome-by-genome shared-family matrices: pdl_genome_matrix (device time between its HIP events, and the wall time of
the whole call: the profile's validation, uploads, launches and the copies back) against the numpy formulation
(pangenome.genome_matrix_host, wall time), on one GPU, in one process, the two roads alternating round by round.  Both must give
the same matrices, or the tool fails.

Sets:
  mycoplasma64_standin            the families of the 64-genome stand-in (tests/golden/net/mycoplasma64_standin.clus.gz over the
                                  names of pandelos_amd.synth's set)
  synthetic_512x5000x350          tools/pan_curves_time.py's labelling: pandelos_amd.synth's family model (round(5000 / 0.85)
                                  families, each present in a genome with probability 0.85, seed 5001) without the residues
  synthetic_2048x5000x350         the same model over 2048 genomes
  ..._copies                      the two synthetic sets with every present family in 1-4 copies (uniform, the model's generator
                                  carried on), so that the extras slabs carry weight

Per set: --warmup + --rounds rounds (default 3 + 20) of each road; median, min, max, p10 and p90 of every figure, whether the
p10-p90 ranges of the two wall times overlap, and the AND-popcount word pairs per second of device time (G * (G + 1) / 2 genome
pairs, mirror included once, over W words; `shared` takes the presence words a second time only as a second atomic, not as a
second product).  A host formulation that takes more than --host-once-above seconds (default 60) is timed once, in front of the
device's rounds, and the device's rounds then run alone.

usage: python tools/genome_matrix_time.py [--set NAME ...] [--out profiles/genome_matrix_time.json]
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
SETS = ("mycoplasma64_standin", "synthetic_512x5000x350", "synthetic_512x5000x350_copies", "synthetic_2048x5000x350",
        "synthetic_2048x5000x350_copies")


def load(name: str, tmp: Path):
    """-> (family_of, genome_of, G)."""
    from pan_curves_time import load as load_profile_set
    if name == "mycoplasma64_standin":
        return load_profile_set(name, tmp)
    from pandelos_amd.synth import CONFIGS
    shape = dict(CONFIGS["synthetic_512x5000x350"])
    shape["genomes"] = int(name.split("_")[1].split("x")[0])
    rng = np.random.Generator(np.random.PCG64(shape["seed"]))
    presence = 0.85
    fams = int(round(shape["genes_per_genome"] / presence))
    planted = [np.nonzero(rng.random(fams) < presence)[0] for _ in range(shape["genomes"])]
    if name.endswith("_copies"):
        planted = [np.repeat(p, rng.integers(1, 5, len(p))) for p in planted]
    fam = np.concatenate(planted)
    gen = np.concatenate([np.full(len(p), g, np.uint32) for g, p in enumerate(planted)])
    first = np.full(fams, len(fam), np.int64)
    np.minimum.at(first, fam, np.arange(len(fam)))                    # a family's label: its first gene
    return first[fam].astype(np.uint32), gen, shape["genomes"]


def same(a: dict, b: dict) -> bool:
    return np.array_equal(a["shared"], b["shared"]) and np.array_equal(a["shared_copies"], b["shared_copies"])


def measure(name: str, nat, warmup: int, rounds: int, host_once_above: float, tmp: Path) -> dict:
    from pan_curves_time import stats
    from pandelos_amd import pangenome
    family_of, genome_of, G = load(name, tmp)
    prof = nat.family_profile(family_of, genome_of, G)
    dev_ms, dev_wall, host_wall = [], [], []
    t0 = time.perf_counter()
    want = pangenome.genome_matrix_host(prof)
    first_host = time.perf_counter() - t0
    host_once = first_host > host_once_above
    print(f"[{name}] host formulation: {first_host:.1f} s{' (timed once)' if host_once else ''}", file=sys.stderr, flush=True)
    if host_once:
        host_wall.append(first_host * 1e3)
    for i in range(warmup + rounds):
        t0 = time.perf_counter()
        got = nat.genome_matrix(prof)
        t1 = time.perf_counter()
        if not host_once:
            want = pangenome.genome_matrix_host(prof)
        t2 = time.perf_counter()
        if not same(got, want):
            raise SystemExit(f"{name}: the device's matrices differ from the host's")
        if i >= warmup:
            dev_ms.append(got["device_ms"]); dev_wall.append((t1 - t0) * 1e3)
            if not host_once:
                host_wall.append((t2 - t1) * 1e3)
        print(f"[{name}] round {i + 1} of {warmup + rounds}: device {(t1 - t0) * 1e3:.1f} ms, host {(t2 - t1) * 1e3 if not host_once else first_host * 1e3:.1f} ms",
              file=sys.stderr, flush=True)
    words = -(-got["levels"] // 64)
    pairs = G * (G + 1) // 2 * words
    tiles = -(-G // 64)
    out = {"set": name, "genes": int(len(family_of)), "genomes": int(G), "families": int(prof["families"]), "incidences": int(prof["incidences"]),
           "levels": int(got["levels"]), "words_per_genome": int(words), "slabs": int(got["slabs"]), "splits": int(got["splits"]),
           "word_pairs": int(pairs), "word_pairs_computed": int(tiles * (tiles + 1) // 2 * 64 * 64 * words),
           "genome_matrix_device_ms": stats(dev_ms), "genome_matrix_wall_ms": stats(dev_wall), "genome_matrix_host_wall_ms": stats(host_wall),
           "host_timed_once": bool(host_once), "same_matrices": True}
    out["word_pairs_per_s_device"] = pairs / (out["genome_matrix_device_ms"]["median"] * 1e-3)
    out["word_pairs_computed_per_s_device"] = out["word_pairs_computed"] / (out["genome_matrix_device_ms"]["median"] * 1e-3)
    out["p10_p90_ranges_overlap"] = not (out["genome_matrix_wall_ms"]["p90"] < out["genome_matrix_host_wall_ms"]["p10"]
                                          or out["genome_matrix_host_wall_ms"]["p90"] < out["genome_matrix_wall_ms"]["p10"])
    out["device_road_faster"] = bool(out["genome_matrix_wall_ms"]["median"] < out["genome_matrix_host_wall_ms"]["median"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", nargs="+", default=list(SETS), choices=list(SETS))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--host-once-above", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.open()
    res = []
    with tempfile.TemporaryDirectory() as d:
        for name in args.set:
            r = measure(name, nat, args.warmup, args.rounds, args.host_once_above, Path(d))
            res.append(r)
            print(json.dumps(r), flush=True)
            if args.out:                               # (after every set: a long run leaves what it has)
                Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    nat.close()


if __name__ == "__main__":
    main()
