#!/usr/bin/env python3
"""Time the pan / core accumulation curves over random genome orders: pdl_pan_curves (device time between its HIP events, and the
wall time of the whole call: the profile's validation, uploads, launches and the copies back) against the numpy formulation
(pangenome.pan_curves_host, wall time), on one GPU, in one process, the two roads alternating round by round.  Both must give
the same curves, or the tool fails.

Sets:
  mycoplasma64_standin     the families of the 64-genome stand-in (tests/golden/net/mycoplasma64_standin.clus.gz over the names
                           of pandelos_amd.synth's set)
  synthetic_512x5000x350   a labelling in the shape of BASELINE.json configs[4]: pandelos_amd.synth's family model (round(5000 /
                           0.85) families, each present in a genome with probability 0.85, seed 5001) without the residues

Per set: --orders orders (default 1000, seed 1), --warmup + --rounds rounds (default 3 + 20) of each road; median, min, max, p10
and p90 of every figure, whether the p10-p90 ranges of the two wall times overlap; the profile call's times beside them.

usage: python tools/pan_curves_time.py [--set NAME ...] [--out profiles/pan_curves_time.json]
"""
from __future__ import annotations

import argparse
import gzip
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
GOLDEN = ROOT / "tests" / "golden"
SETS = ("mycoplasma64_standin", "synthetic_512x5000x350")


def stats(xs):
    a = np.asarray(xs, np.float64)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()),
            "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90)), "n": int(len(a))}


def load(name: str, tmp: Path):
    """-> (family_of, genome_of, G)."""
    from pandelos_amd import netclu, pangenome
    from pandelos_amd.synth import CONFIGS, make_gene_set
    shape = CONFIGS[name]
    if name == "mycoplasma64_standin":
        faa = tmp / f"{name}.faa"
        make_gene_set(**shape).write_faa(faa)
        names, genome_of = netclu.read_names(faa)
        gen, genome_names = pangenome.genome_ids(genome_of)
        return pangenome.family_of_from_clus(names, gzip.open(GOLDEN / "net" / f"{name}.clus.gz", "rt").read()), gen, len(genome_names)
    rng = np.random.Generator(np.random.PCG64(shape["seed"]))
    presence = 0.85
    fams = int(round(shape["genes_per_genome"] / presence))
    planted = [np.nonzero(rng.random(fams) < presence)[0] for _ in range(shape["genomes"])]
    fam = np.concatenate(planted)
    gen = np.concatenate([np.full(len(p), g, np.uint32) for g, p in enumerate(planted)])
    first = np.full(fams, len(fam), np.int64)
    np.minimum.at(first, fam, np.arange(len(fam)))                    # a family's label: its first gene
    return first[fam].astype(np.uint32), gen, shape["genomes"]


def measure(name: str, nat, n_orders: int, warmup: int, rounds: int, tmp: Path) -> dict:
    from pandelos_amd import pangenome
    family_of, genome_of, G = load(name, tmp)
    prof_wall, prof_dev = [], []
    for i in range(warmup + rounds):
        t0 = time.perf_counter()
        prof = nat.family_profile(family_of, genome_of, G)
        if i >= warmup:
            prof_wall.append((time.perf_counter() - t0) * 1e3)
            prof_dev.append(nat.last_profile_info["device_ms"])
    orders = pangenome.random_orders(G, n_orders, 1)
    dev_ms, dev_wall, host_wall = [], [], []
    for i in range(warmup + rounds):
        t0 = time.perf_counter()
        got = nat.pan_curves(prof, orders)
        t1 = time.perf_counter()
        want = pangenome.pan_curves_host(prof, orders)
        t2 = time.perf_counter()
        if not (np.array_equal(got["pan"], want["pan"]) and np.array_equal(got["core"], want["core"])):
            raise SystemExit(f"{name}: the device's curves differ from the host's")
        if i >= warmup:
            dev_ms.append(nat.last_curves_info["device_ms"]); dev_wall.append((t1 - t0) * 1e3); host_wall.append((t2 - t1) * 1e3)
        print(f"[{name}] round {i + 1} of {warmup + rounds}: device {(t1 - t0) * 1e3:.1f} ms, host {(t2 - t1) * 1e3:.1f} ms", file=sys.stderr, flush=True)
    out = {"set": name, "genes": int(len(family_of)), "genomes": int(G), "families": int(prof["families"]), "incidences": int(prof["incidences"]),
           "core": int(prof["core"]), "accessory": int(prof["accessory"]), "unique": int(prof["unique"]), "orders": int(n_orders),
           "steps_orders_x_incidences": int(n_orders) * int(prof["incidences"]),
           "pan_curves_device_ms": stats(dev_ms), "pan_curves_wall_ms": stats(dev_wall), "pan_curves_host_wall_ms": stats(host_wall),
           "family_profile_device_ms": stats(prof_dev), "family_profile_wall_ms": stats(prof_wall), "same_curves": True}
    out["p10_p90_ranges_overlap"] = not (out["pan_curves_wall_ms"]["p90"] < out["pan_curves_host_wall_ms"]["p10"]
                                          or out["pan_curves_host_wall_ms"]["p90"] < out["pan_curves_wall_ms"]["p10"])
    out["device_road_faster"] = bool(out["pan_curves_wall_ms"]["median"] < out["pan_curves_host_wall_ms"]["median"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", nargs="+", default=list(SETS), choices=list(SETS))
    ap.add_argument("--orders", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.open()
    res = []
    with tempfile.TemporaryDirectory() as d:
        for name in args.set:
            r = measure(name, nat, args.orders, args.warmup, args.rounds, Path(d))
            res.append(r)
            print(json.dumps(r), flush=True)
            if args.out:                               # (after every set: a long run leaves what it has)
                Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    nat.close()


if __name__ == "__main__":
    main()
