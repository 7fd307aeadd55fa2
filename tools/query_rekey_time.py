#!/usr/bin/env python3
"""Time pdl_query_scores for a genome that brings a letter the base lacks (option "query_rekey") against the only road to that
block before: the union rebuild and a full scoring pass, on one GPU.  Shape and protocol of tools/rekey_time.py.

For a set of pandelos_amd.synth.CONFIGS the last genome is held out and ONE of its residues is replaced by a letter the rest of
the set lacks.  Contexts in one process, "stage_timers" 0:
  rekey   the dictionary of the other G-1 genomes with the option on (NOT timed), then timed: pdl_query_scores of the held-out
          genome with the letter (wall time of the call and pdl_query_info.device_ms)
  plain   the same context: the held-out genome WITHOUT the letter — what the alphabet change adds
  union   timed: pdl_preprocess + pdl_score_all of the whole set with the letter (wall time; device time = preprocess_total_ms
          + score_total_ms) — by the library given with --baseline-lib (a libpandelos_amd.so built from the parent commit in a side
          directory), else by this library
Warm-up first, then the three alternate --repeat times; median, min, max and the 10th / 90th percentiles of each.  Bar: the
re-keyed query's p90 below the rebuild's p10.  The rebase pass's own time comes from --split-repeat further queries with
"stage_timers" 1 (pdl_query_rekey_info.rebase_ms).  After the timing the re-keyed block is compared, field by field, with
pdl_compute_scores(G) of a union build of this library.

usage: python tools/query_rekey_time.py [--config mycoplasma64_standin synthetic_128x4000x300] [--baseline-lib PATH] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tools.append_time import FIELDS, stats  # noqa: E402
from tools.query_time import split_last_genome  # noqa: E402
from tools.remove_time import open_with_library  # noqa: E402


def measure(config: str, repeat: int, warmup: int, split_repeat: int, check: bool, baseline_lib) -> dict:
    from pandelos_amd.calculate_k import calculate_k
    from pandelos_amd.pangene_native import PangeneNative
    from pandelos_amd.synth import CONFIGS, make_gene_set
    gs = make_gene_set(**CONFIGS[config])
    k = calculate_k(gs.residues)
    base, query, union = split_last_genome(gs)
    present = np.zeros(256, bool)
    present[gs.residues] = True
    letter = next(b for b in b"XUBZOJ*" if not present[b])           # a letter the set lacks
    qx = query[0].copy()
    lens = np.diff(query[1].astype(np.int64))
    gene = int(np.argmax(lens >= k))                                 # ... in the middle of the first gene that has a k-mer
    qx[int(query[1][gene]) + int(lens[gene]) // 2] = letter
    query_x = (qx, query[1])
    union_x = (np.concatenate([base[0], qx]), union[1], union[2])

    nb = PangeneNative.open()
    nb.set_option("stage_timers", 0); nb.set_option("query_rekey", 1)
    nb.preprocess(k, *base)                                          # the base build: outside the timed region
    nu = open_with_library(baseline_lib) if baseline_lib else PangeneNative.open()
    if baseline_lib:
        nu._lib.pdl_score_all.argtypes = [C.c_void_p]; nu._lib.pdl_score_all.restype = C.c_int
    nu.set_option("stage_timers", 0)

    def run_query(genes):
        t0 = time.perf_counter()
        s = nb.query_scores(*genes)
        return (time.perf_counter() - t0) * 1e3, nb.last_query_info["device_ms"], s

    def run_union():
        t0 = time.perf_counter()
        nu.preprocess(k, *union_x)
        nu.score_all()
        wall = (time.perf_counter() - t0) * 1e3
        tm = nu.timings()
        return wall, tm["preprocess_total_ms"] + tm["score_total_ms"]

    for _ in range(warmup):
        run_query(query_x); run_union(); run_query(query)
    r_wall, r_dev, u_wall, u_dev, p_wall, p_dev = [], [], [], [], [], []
    block = None
    for _ in range(repeat):
        w, d, block = run_query(query_x)
        r_wall.append(w); r_dev.append(d)
        w, d = run_union()
        u_wall.append(w); u_dev.append(d)
        w, d, _ = run_query(query)
        p_wall.append(w); p_dev.append(d)
    run_query(query_x)
    info, ri = dict(nb.last_query_info), nb.last_query_rekey_info
    assert ri["queries_rekeyed"] == 1, ri
    nb.set_option("stage_timers", 1)
    rebase_ms, timed_dev = [], []
    for _ in range(split_repeat):
        _, d, _ = run_query(query_x)
        rebase_ms.append(nb.last_query_rekey_info["rebase_ms"]); timed_dev.append(d)
    out = {
        "config": config, "shape": CONFIGS[config], "k": k, "new_letter": chr(letter),
        "baseline": "parent commit's library" if baseline_lib else "this library",
        "query_rekey_info": ri,
        "query": {"genes": int(len(query[1]) - 1), "cells": int(block.scoresCount),
                  **{kk: info[kk] for kk in ("residues", "kmer_occurrences", "records", "matched_records", "genome_cost")}},
        "rekey_query_device_ms": stats(r_dev), "rekey_query_wall_ms": stats(r_wall),
        "plain_query_device_ms": stats(p_dev), "plain_query_wall_ms": stats(p_wall),
        "union_rebuild_device_ms": stats(u_dev), "union_rebuild_wall_ms": stats(u_wall),
        "stage_timers_on": {"rebase_ms": stats(rebase_ms), "rekey_query_device_ms": stats(timed_dev)},
    }
    r, u, p = out["rekey_query_device_ms"], out["union_rebuild_device_ms"], out["plain_query_device_ms"]
    out["device_ratio_median"] = r["median"] / u["median"]
    out["rekey_over_plain_query_median"] = r["median"] / p["median"]
    out["rekey_faster_ranges_apart"] = bool(r["p90"] < u["p10"])
    rw, uw = out["rekey_query_wall_ms"], out["union_rebuild_wall_ms"]
    out["rekey_faster_ranges_apart_wall"] = bool(rw["p90"] < uw["p10"])
    if check:
        fresh = PangeneNative.open()
        fresh.preprocess(k, *union_x)
        G = int(fresh.cost.genomes) - 1
        want, got = fresh.generate_scores_part(G).as_dict(), block.as_dict()
        same = all(np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(want[f]).tobytes() for f in FIELDS) \
            and int(got["scoresCount"]) == int(want["scoresCount"]) and info["genome_cost"] == fresh.genome_cost(G)
        out["union_block_check"] = "match" if same else "MISMATCH"
        fresh.close()
    nb.close(); nu.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["mycoplasma64_standin", "synthetic_128x4000x300"])
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--split-repeat", type=int, default=5)
    ap.add_argument("--no-check", action="store_true", help="do not compare the block with a union build's")
    ap.add_argument("--baseline-lib", default=None, help="libpandelos_amd.so of the parent commit (default: this library rebuilds)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = []
    for c in args.config:
        r = measure(c, args.repeat, args.warmup, args.split_repeat, not args.no_check, args.baseline_lib)
        res.append(r)
        print(json.dumps({kk: r.get(kk) for kk in ("config", "device_ratio_median", "rekey_over_plain_query_median", "rekey_faster_ranges_apart",
                                                   "rekey_faster_ranges_apart_wall", "union_block_check")}), flush=True)
        print(json.dumps({"rekey_query_device_ms": r["rekey_query_device_ms"], "plain_query_device_ms": r["plain_query_device_ms"],
                          "union_rebuild_device_ms": r["union_rebuild_device_ms"], "rebase_ms": r["stage_timers_on"]["rebase_ms"]}), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
