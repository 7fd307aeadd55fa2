#!/usr/bin/env python3
"""Time pdl_query_scores against the rebuild it replaces, on one GPU.

For a set of pandelos_amd.synth.CONFIGS, the last genome is held out as the query.  Two contexts:
  base   the dictionary of the other genomes; timed: pdl_query_scores (wall time of the call and its device_ms)
  union  timed: pdl_preprocess + pdl_score_all of the whole set with "stage_timers" 0 (wall time; device time =
         preprocess_total_ms + score_total_ms of pdl_timings)
Warm-up first, then the two alternate --repeat times; median, min, max and the 10th / 90th percentiles of each.

usage: python tools/query_time.py [--config mycoplasma64_standin synthetic_128x4000x300] [--repeat 20] [--out FILE]
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
    held = int(gs.genome_of.max())
    off = gs.offsets.astype(np.int64)
    base_ids = np.nonzero(gs.genome_of != held)[0]
    query_ids = np.nonzero(gs.genome_of == held)[0]

    def pack(ids):
        lens = off[ids + 1] - off[ids]
        o = np.zeros(len(ids) + 1, np.uint64)
        np.cumsum(lens, out=o[1:])
        r = np.concatenate([gs.residues[off[i]:off[i + 1]] for i in ids]).astype(np.uint8)
        return r, o
    rb, ob_ = pack(base_ids)
    rq, oq = pack(query_ids)
    gb = gs.genome_of[base_ids].astype(np.uint32)        # (synth sets are genome-major: ids stay dense)
    res = np.concatenate([rb, rq])
    off_u = np.concatenate([ob_, ob_[-1] + oq[1:]]).astype(np.uint64)
    gen_u = np.concatenate([gb, np.full(len(query_ids), held, np.uint32)])
    return (rb, ob_, gb), (rq, oq), (res, off_u, gen_u)


def measure(config: str, repeat: int, warmup: int) -> dict:
    from pandelos_amd.calculate_k import calculate_k
    from pandelos_amd.pangene_native import PangeneNative
    from pandelos_amd.synth import CONFIGS, make_gene_set
    gs = make_gene_set(**CONFIGS[config])
    k = calculate_k(gs.residues)
    base, query, union = split_last_genome(gs)
    nb = PangeneNative.open()
    nb.set_option("stage_timers", 0)
    nb.preprocess(k, *base)
    nu = PangeneNative.open()
    nu.set_option("stage_timers", 0)

    def run_query():
        t0 = time.perf_counter()
        s = nb.query_scores(*query)
        return (time.perf_counter() - t0) * 1e3, nb.last_query_info["device_ms"], s.scoresCount

    def run_union():
        t0 = time.perf_counter()
        nu.preprocess(k, *union)
        nu.score_all()
        wall = (time.perf_counter() - t0) * 1e3
        tm = nu.timings()
        return wall, tm["preprocess_total_ms"] + tm["score_total_ms"]

    for _ in range(warmup):
        run_query()
        run_union()
    q_wall, q_dev, u_wall, u_dev = [], [], [], []
    cells = 0
    for _ in range(repeat):
        w, d, cells = run_query()
        q_wall.append(w); q_dev.append(d)
        w, d = run_union()
        u_wall.append(w); u_dev.append(d)
    info = dict(nb.last_query_info)
    out = {
        "config": config, "shape": CONFIGS[config], "k": k,
        "base": {"sequences": int(nb.cost.sequences), "genomes": int(nb.cost.genomes), "records": int(nb.cost.dictionary_records)},
        "query": {"genes": int(len(query[1]) - 1), "cells": int(cells), **{kk: info[kk] for kk in ("residues", "kmer_occurrences", "records", "matched_records", "genome_cost")}},
        "union_total_cost": int(nu.cost.total_cost),
        "query_device_ms": stats(q_dev), "query_wall_ms": stats(q_wall),
        "union_rebuild_device_ms": stats(u_dev), "union_rebuild_wall_ms": stats(u_wall),
    }
    out["device_ratio_median"] = out["query_device_ms"]["median"] / out["union_rebuild_device_ms"]["median"]
    out["wall_ratio_median"] = out["query_wall_ms"]["median"] / out["union_rebuild_wall_ms"]["median"]
    out["target_quarter_met"] = bool(out["device_ratio_median"] <= 0.25)
    nb.close(); nu.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["mycoplasma64_standin", "synthetic_128x4000x300"])
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = []
    for c in args.config:
        r = measure(c, args.repeat, args.warmup)
        res.append(r)
        print(json.dumps({kk: r[kk] for kk in ("config", "device_ratio_median", "wall_ratio_median", "target_quarter_met")}), flush=True)
        print(json.dumps({"query_device_ms": r["query_device_ms"], "union_rebuild_device_ms": r["union_rebuild_device_ms"]}), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
