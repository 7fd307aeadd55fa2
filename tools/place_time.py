#!/usr/bin/env python3
"""Time K-place (pdl_place_query) against the road that exists without it, on one GPU, in one process.

Per config of pandelos_amd.synth.CONFIGS (default: the canonical 64-genome set and configs[3]) the last genome is held out as the
query.  After --warmup rounds, --repeat rounds, the three alternating inside a round:
  place       pdl_place_query on a base that has its scores, edges and families: device_ms and the wall time of the call
  query       pdl_query_scores alone on the same base: device_ms and wall time — what K-place adds is the difference
  commit      today's road on a FRESH copy of the base (preprocess and scoring pass of the base not timed): pdl_append_genomes,
              pdl_score_all, pdl_compute_families — device time (the append's device_ms + the scoring pass's score_total_ms +
              K-fam's device_ms; K-bbh of the union is not in it) and wall time of the three calls
Median, min, max, 10th / 90th percentile of each, the counts, whether the p10-p90 ranges of place and commit overlap and which is
faster — whichever way it comes out.  --commit-repeat / --commit-warmup: fewer rounds of the commit road (each needs a base rebuilt).

usage: python tools/place_time.py [--config NAME ...] [--repeat 20] [--warmup 3] [--out profiles/place_time.json]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def stats(xs):
    a = np.asarray(xs, np.float64)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()),
            "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90)), "n": int(len(a))}


def split_last_genome(gs):
    gen = np.asarray(gs.genome_of)
    off = np.asarray(gs.offsets, np.uint64)
    first = int(np.searchsorted(gen, int(gen.max())))            # (synthetic sets hold their genomes one behind the other)
    assert (gen[first:] == gen.max()).all() and (gen[:first] < gen.max()).all()
    cut = int(off[first])
    return (gs.residues[:cut], off[:first + 1], gen[:first]), (gs.residues[cut:], off[first:] - off[first])


def overlap(a, b):
    return not (a["p90"] < b["p10"] or b["p90"] < a["p10"])


def measure(config: str, repeat: int, warmup: int, commit_repeat: int, commit_warmup: int) -> dict:
    from pandelos_amd.calculate_k import calculate_k
    from pandelos_amd.pangene_native import PangeneNative
    from pandelos_amd.synth import CONFIGS, make_gene_set
    gs = make_gene_set(**CONFIGS[config])
    k = calculate_k(gs.residues)
    base, query = split_last_genome(gs)
    nat = PangeneNative.from_arrays(k, *base)
    nat.generate_families()                                       # scores, edges, families of the base: not timed
    fresh = PangeneNative.open()
    place, qry, commit = [], [], []
    last = {}

    def one_place():
        t0 = time.perf_counter()
        pl = nat.place_query(*query)
        wall = (time.perf_counter() - t0) * 1e3
        last["place"] = pl
        return wall, nat.last_place_info["device_ms"], nat.last_place_info["query"]["device_ms"]

    def one_query():
        t0 = time.perf_counter()
        nat.query_scores(*query)
        return (time.perf_counter() - t0) * 1e3, nat.last_query_info["device_ms"]

    def one_commit():
        fresh.preprocess(k, *base)
        fresh.score_all()
        t0 = time.perf_counter()
        fresh.append(*query)
        fresh.score_all()
        fresh.generate_families()
        wall = (time.perf_counter() - t0) * 1e3
        return wall, fresh.last_append_info["device_ms"] + fresh.timings()["score_total_ms"] + fresh.last_families_info["device_ms"]

    print(f"[{config}] {len(base[2])} base genes, {len(query[1]) - 1} query genes, k = {k}", file=sys.stderr, flush=True)
    for r in range(-warmup, repeat):
        p, q = one_place(), one_query()
        c = one_commit() if r + warmup < commit_warmup + commit_repeat else None
        if r >= 0:
            place.append(p); qry.append(q)
        if c is not None and r + warmup >= commit_warmup:
            commit.append(c)
    pl = last["place"]
    out = {"config": config, "shape": CONFIGS[config], "k": int(k), "base_genes": int(len(base[2])), "query_genes": int(len(query[1]) - 1),
           "edges": int(len(pl["src"])), **{f: int(pl[f]) for f in ("edges_phase1", "groups", "novel", "joined", "bridging", "colliding", "unplaced")},
           "place_device_ms": stats([d for _, d, _ in place]), "place_wall_ms": stats([w for w, _, _ in place]),
           "place_query_part_device_ms": stats([q for _, _, q in place]),
           "kplace_added_device_ms": stats([d - q for _, d, q in place]),
           "query_device_ms": stats([d for _, d in qry]), "query_wall_ms": stats([w for w, _ in qry]),
           "commit_device_ms": stats([d for _, d in commit]), "commit_wall_ms": stats([w for w, _ in commit])}
    for unit in ("device", "wall"):
        a, b = out[f"place_{unit}_ms"], out[f"commit_{unit}_ms"]
        out[f"{unit}_p10_p90_ranges_overlap"] = overlap(a, b)
        out[f"{unit}_faster"] = "place" if a["median"] < b["median"] else "commit"
    nat.close(); fresh.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["mycoplasma64_standin", "synthetic_128x4000x300"])
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--commit-repeat", type=int, default=None)
    ap.add_argument("--commit-warmup", type=int, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = []
    for c in args.config:
        r = measure(c, args.repeat, args.warmup, args.repeat if args.commit_repeat is None else args.commit_repeat,
                    args.warmup if args.commit_warmup is None else args.commit_warmup)
        res.append(r)
        print(json.dumps(r), flush=True)
        if args.out:                               # (after every config: a long run leaves what it has)
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
