#!/usr/bin/env python3
"""Time K-fam (pdl_compute_families) and the .faa -> .clus road that uses it against the host road it replaces, on one GPU, in
one process.

Per config of pandelos_amd.synth.CONFIGS (default: the canonical 64-genome set and configs[3]), after --warmup rounds, --repeat
rounds of each:
  kfam        pdl_compute_families alone on a context that has its edges (scoring pass and K-bbh done and not timed; the cache is
              dropped by scoring again): its device_ms and the wall time of the call
  new road    .faa -> ingest -> preprocess -> families on the device -> netclu.families_from_components -> .clus written
  host road   .faa -> ingest -> preprocess -> pdl_compute_edges -> net_lines -> .net written -> read_net -> families -> .clus written
Both roads must write the same bytes.  Median, min, max, 10th / 90th percentile of each, the counts, and whether the two roads'
p10-p90 ranges overlap.  --host-repeat / --host-warmup: fewer rounds of the host road (it takes tens of seconds on configs[3]).

usage: python tools/families_time.py [--config NAME ...] [--repeat 20] [--warmup 3] [--out profiles/families_time.json]
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


def stats(xs):
    a = np.asarray(xs, np.float64)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()),
            "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90)), "n": int(len(a))}


def measure(config: str, repeat: int, warmup: int, host_repeat: int, host_warmup: int, tmp: Path) -> dict:
    from pandelos_amd import families as FAM
    from pandelos_amd import netclu
    from pandelos_amd.calculate_k import calculate_k
    from pandelos_amd.pangene_native import PangeneNative
    from pandelos_amd.pangenes import net_lines
    from pandelos_amd.synth import CONFIGS, make_gene_set
    gs = make_gene_set(**CONFIGS[config])
    k = calculate_k(gs.residues)
    faa = tmp / f"{config}.faa"
    gs.write_faa(faa)
    nat = PangeneNative.open()
    last = {}

    def start():
        ing = nat.ingest_faa(faa)
        nat.preprocess_ingested(k)
        return ing, netclu.read_names(faa)

    def new_road():
        t0 = time.perf_counter()
        ing, (names, genome_of) = start()
        text, fam, _ = FAM.clus_from_native(nat, names, genome_of, ing["genomes"])
        (tmp / "new.clus").write_text(text)
        last["new"] = text
        return (time.perf_counter() - t0) * 1e3

    def host_road():
        t0 = time.perf_counter()
        ing, (names, genome_of) = start()
        src, dst, sc = FAM.gather_edges(nat, ing["genomes"])
        with open(tmp / "host.net", "w") as f:
            f.writelines(net_lines(src, dst, sc))
        fams, singles = netclu.families(names, genome_of, netclu.read_net(tmp / "host.net"))
        text = netclu.clus_text(names, fams, singles)
        (tmp / "host.clus").write_text(text)
        last["host"], last["edges"] = text, int(len(src))
        return (time.perf_counter() - t0) * 1e3

    def kfam():
        nat.set_option("stage_timers", 1)              # (the default value; any option change drops scores, edges and families)
        nat.generate_edges_part(0)                     # the scoring pass and K-bbh, not timed
        t0 = time.perf_counter()
        nat.generate_families()
        return (time.perf_counter() - t0) * 1e3, nat.last_families_info["device_ms"]

    def rounds(what, fn, n_warm, n):
        for _ in range(n_warm):
            fn()
        out = [fn() for _ in range(n)]
        print(f"[{config}] {what}: {n_warm} + {n} rounds done", file=sys.stderr, flush=True)
        return out

    print(f"[{config}] {gs.genes} genes written, k = {k}", file=sys.stderr, flush=True)
    new_wall = rounds("new road", new_road, warmup, repeat)
    kf = rounds("kfam", kfam, warmup, repeat)
    host_wall = rounds("host road", host_road, host_warmup, host_repeat)
    info = dict(nat.last_families_info)
    out = {"config": config, "shape": CONFIGS[config], "k": int(k), "edges": last["edges"],
           **{f: int(info[f]) for f in ("sequences", "nodes", "families", "colliding")},
           "kfam_device_ms": stats([d for _, d in kf]), "kfam_wall_ms": stats([w for w, _ in kf]),
           "new_road_wall_ms": stats(new_wall), "host_road_wall_ms": stats(host_wall),
           "same_clus": last["new"] == last["host"]}
    out["new_road_faster"] = bool(out["new_road_wall_ms"]["median"] < out["host_road_wall_ms"]["median"])
    out["p10_p90_ranges_overlap"] = not (out["new_road_wall_ms"]["p90"] < out["host_road_wall_ms"]["p10"]
                                          or out["host_road_wall_ms"]["p90"] < out["new_road_wall_ms"]["p10"])
    nat.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["mycoplasma64_standin", "synthetic_128x4000x300"])
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-repeat", type=int, default=None)
    ap.add_argument("--host-warmup", type=int, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = []
    with tempfile.TemporaryDirectory() as d:
        for c in args.config:
            r = measure(c, args.repeat, args.warmup, args.repeat if args.host_repeat is None else args.host_repeat,
                        args.warmup if args.host_warmup is None else args.host_warmup, Path(d))
            res.append(r)
            print(json.dumps(r), flush=True)
            if args.out:                               # (after every config: a long run leaves what it has)
                Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
