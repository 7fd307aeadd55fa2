#!/usr/bin/env python3
"""Time the Girvan-Newman split of all colliding components of a network: the host road (netclu.split_until_clean per component)
against the device road (netclu.split_all_until_clean with the device splitter — packing, pdl_split_first_level and the host
glue of every level included), on one GPU, in one process.  Both must give the same partition, or the tool fails.

Sets (warm-ups + rounds of each road; --host-warmup / --host-repeat / --warmup / --repeat override them for every set named):
  paralogs_10x60x90_k3_div20   tests/golden/net, components of at most 16 genes            3 + 20
  community_100, community_200 tests/golden/split, one two-community component each        3 + 20
  community_400                generated (tests/split_cases.two_community_edges)           device 3 + 20, host 1 + 3 (a host round
                                                                                           takes minutes)

Per set: median, min, max, p10, p90 of both roads' wall time, whether the p10-p90 ranges overlap, the device's counts and its
device_ms per betweenness round.

usage: python tools/split_time.py [--set NAME ...] [--out profiles/split_time.json]
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
GOLDEN = ROOT / "tests" / "golden"
ROUNDS = {"paralogs_10x60x90_k3_div20": (3, 20, 3, 20), "community_100": (3, 20, 3, 20), "community_200": (3, 20, 3, 20),
          "community_400": (3, 20, 1, 3)}          # device warm-ups, rounds; host warm-ups, rounds


def stats(xs):
    a = np.asarray(xs, np.float64)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()),
            "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90)), "n": int(len(a))}


def load(name: str, tmp: Path):
    """-> (adjacency, genome labels) of a set."""
    from pandelos_amd import netclu
    if name.startswith("paralogs"):
        from pandelos_amd.synth import make_gene_set
        from tests.test_host_net import CASES
        faa = tmp / f"{name}.faa"
        make_gene_set(**CASES[name][0]).write_faa(faa)
        return netclu.read_net(GOLDEN / "net" / f"{name}.net"), netclu.read_names(faa)[1]
    if name == "community_400":
        from tests.split_cases import two_community_edges
        adj = {}
        for a, b in two_community_edges(400, 400):
            adj.setdefault(a, {}); adj.setdefault(b, {})
            adj[a][b] = None
            adj[b][a] = None
        return adj, [f"genome{g % 16:02d}" for g in range(400)]
    return netclu.read_net(GOLDEN / "split" / f"{name}.net"), netclu.read_names(GOLDEN / "split" / f"{name}.faa")[1]


def measure(name: str, nat, rounds, tmp: Path) -> dict:
    from pandelos_amd import families as FAM
    from pandelos_amd import netclu
    adj, genome_of = load(name, tmp)
    comps = [c for c in netclu.connected_components(adj) if netclu.max_collision(c, adj, genome_of) > 0]
    last = {}

    def filters():
        return [netclu.view_filter(c, adj.__contains__) for c in comps]

    def host_road():
        fs = filters()
        t0 = time.perf_counter()
        last["host"] = [netclu.split_until_clean(f, adj, genome_of) for f in fs]
        return (time.perf_counter() - t0) * 1e3

    def device_road():
        fs, splitter = filters(), FAM.DeviceSplitter(nat)
        t0 = time.perf_counter()
        last["device"] = netclu.split_all_until_clean(fs, adj, genome_of, None, splitter)
        last["totals"] = splitter.totals
        return (time.perf_counter() - t0) * 1e3

    def run(what, fn, n_warm, n):
        out = []
        for i in range(n_warm + n):
            ms = fn()
            if i >= n_warm:
                out.append(ms)
            if ms > 10e3:                              # (a long round says so: minutes without a line look like a hang)
                print(f"[{name}] {what}: round {i + 1} of {n_warm + n}, {ms / 1e3:.1f} s", file=sys.stderr, flush=True)
        print(f"[{name}] {what}: {n_warm} + {n} rounds done, median {np.median(out):.1f} ms", file=sys.stderr, flush=True)
        return out

    dw, dr, hw, hr = rounds
    dev = run("device road", device_road, dw, dr)
    host = run("host road", host_road, hw, hr)
    if last["device"] != last["host"]:
        raise SystemExit(f"{name}: the device road's partition differs from the host road's")
    t = last["totals"]
    out = {"set": name, "nodes": len(adj), "colliding_components": len(comps), "largest_component": max(len(c) for c in comps),
           "device_road_wall_ms": stats(dev), "host_road_wall_ms": stats(host), "same_partition": True,
           "calls": t["calls"], "graphs": t["graphs"], "removals": t["removals"], "rounds": t["rounds"],
           "device_ms": t["device_ms"], "device_ms_per_round": t["device_ms"] / t["rounds"] if t["rounds"] else None}
    out["p10_p90_ranges_overlap"] = not (out["device_road_wall_ms"]["p90"] < out["host_road_wall_ms"]["p10"]
                                          or out["host_road_wall_ms"]["p90"] < out["device_road_wall_ms"]["p10"])
    out["device_road_faster"] = bool(out["device_road_wall_ms"]["median"] < out["host_road_wall_ms"]["median"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", nargs="+", default=list(ROUNDS), choices=list(ROUNDS))
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--repeat", type=int, default=None)
    ap.add_argument("--host-warmup", type=int, default=None)
    ap.add_argument("--host-repeat", type=int, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.open()
    res = []
    with tempfile.TemporaryDirectory() as d:
        for name in args.set:
            rounds = tuple(r if o is None else o for r, o in zip(ROUNDS[name], (args.warmup, args.repeat, args.host_warmup, args.host_repeat)))
            r = measure(name, nat, rounds, Path(d))
            res.append(r)
            print(json.dumps(r), flush=True)
            if args.out:                               # (after every set: a long run leaves what it has)
                Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    nat.close()


if __name__ == "__main__":
    main()
