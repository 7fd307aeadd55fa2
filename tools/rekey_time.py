#!/usr/bin/env python3
"""Time pdl_append_genomes across a change of the alphabet (option "alphabet_rekey") against the rebuild it replaces, on one GPU.

For a set of pandelos_amd.synth.CONFIGS the last genome is held out and ONE of its residues is replaced by a letter the rest of
the set lacks: the union has one letter more than the base, every key of the base's sorted stream changes.  Contexts in one
process, "stage_timers" 0:
  rekey   pdl_preprocess of the other G-1 genomes with the option on (NOT timed), then timed: pdl_append_genomes of the held-out
          genome (wall time of the call and pdl_append_info.device_ms)
  union   timed: pdl_preprocess of the whole set (wall time; device time = pdl_timings.preprocess_total_ms) — by the library given
          with --baseline-lib (a libpandelos_amd.so built from the parent commit in a side directory: before this option the only
          road to this context), else by this library
  plain   the same append of the held-out genome WITHOUT the new letter, by this library: what the re-key adds
Warm-up first, then the three alternate --repeat times; median, min, max and the 10th / 90th percentiles of each.  The re-key
pass's own time comes from --split-repeat further appends with "stage_timers" 1 (pdl_rekey_info.rekey_ms); its TB/s counts the
base's keys once in and once out: (key bytes before + key bytes after) * M.
After the timing the re-keyed context is compared with a union build of this library: pdl_cost, the rank table and the sha256
of every Scores field of --check-genomes genomes (the first ones and the appended one).

--k K forces the k-mer length: 20 letters have 32-bit keys up to k = 7 and exact 64-bit ones up to k = 14 (21 letters: k = 14 too).

usage: python tools/rekey_time.py [--config mycoplasma64_standin synthetic_128x4000x300] [--baseline-lib PATH] [--k K] [--out FILE]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tools.append_time import FIELDS, split_last_genome, stats  # noqa: E402
from tools.remove_time import open_with_library  # noqa: E402


def score_digests(nat, genomes):
    out = {}
    for g in genomes:
        s = nat.generate_scores_part(g).as_dict()
        d = {"scoresCount": int(s["scoresCount"])}
        for f in FIELDS:
            a = np.ascontiguousarray(s[f])
            a = a.view(np.uint32) if a.dtype == np.float32 else a
            d[f] = hashlib.sha256(a.tobytes()).hexdigest()
        out[int(g)] = d
    return out


def measure(config: str, repeat: int, warmup: int, split_repeat: int, check_genomes: int, baseline_lib, k_forced: int = 0) -> dict:
    from pandelos_amd.calculate_k import calculate_k
    from pandelos_amd.pangene_native import PangeneNative
    from pandelos_amd.synth import CONFIGS, make_gene_set
    gs = make_gene_set(**CONFIGS[config])
    k = k_forced or calculate_k(gs.residues)
    base, new = split_last_genome(gs)
    present = np.zeros(256, bool)
    present[gs.residues] = True
    letter = next(b for b in b"XUBZOJ*" if not present[b])           # a letter the set lacks
    new_res = new[0].copy()
    lens = np.diff(new[1].astype(np.int64))
    gene = int(np.argmax(lens >= k))                                 # ... in the middle of the first gene that has a k-mer
    new_res[int(new[1][gene]) + int(lens[gene]) // 2] = letter
    new_x = (new_res, new[1])
    union_x = (np.concatenate([base[0], new_res]), gs.offsets, gs.genome_of)

    nr = PangeneNative.open()
    nr.set_option("stage_timers", 0); nr.set_option("alphabet_rekey", 1)
    npl = PangeneNative.open()
    npl.set_option("stage_timers", 0)
    nu = open_with_library(baseline_lib) if baseline_lib else PangeneNative.open()
    nu.set_option("stage_timers", 0)

    def run_append(nat, genes):
        nat.preprocess(k, *base)                        # the base build: outside the timed region
        t0 = time.perf_counter()
        nat.append(*genes)
        return (time.perf_counter() - t0) * 1e3, nat.last_append_info["device_ms"]

    def run_union():
        t0 = time.perf_counter()
        nu.preprocess(k, *union_x)
        return (time.perf_counter() - t0) * 1e3, nu.timings()["preprocess_total_ms"]

    for _ in range(warmup):
        run_append(nr, new_x); run_union(); run_append(npl, new)
    r_wall, r_dev, u_wall, u_dev, p_wall, p_dev = [], [], [], [], [], []
    for _ in range(repeat):
        w, d = run_append(nr, new_x)
        r_wall.append(w); r_dev.append(d)
        w, d = run_union()
        u_wall.append(w); u_dev.append(d)
        w, d = run_append(npl, new)
        p_wall.append(w); p_dev.append(d)
    ri = nr.last_rekey_info
    assert ri["rekeyed"] == 1 and nr.cost.as_dict() == nu.cost.as_dict(), "the re-keyed context and the union build disagree"
    # the pass itself, with the stage timers on
    nr.set_option("stage_timers", 1)
    rekey_ms, merge_ms, rank_sort_ms = [], [], []
    for _ in range(split_repeat):
        run_append(nr, new_x)
        rekey_ms.append(nr.last_rekey_info["rekey_ms"]); merge_ms.append(nr.last_append_info["merge_ms"]); rank_sort_ms.append(nr.last_append_info["rank_sort_ms"])
    M0 = int(ri["keys_rewritten"])
    kb0, kb1 = (8 if ri["key_bits_before"] > 32 else 4), (8 if ri["key_bits_after"] > 32 else 4)
    rekey_bytes = (kb0 + kb1) * M0
    out = {
        "config": config, "shape": CONFIGS[config], "k": k, "new_letter": chr(letter),
        "baseline": "parent commit's library" if baseline_lib else "this library",
        "rekey_info": ri, "union": {"sequences": int(nr.cost.sequences), "kmer_occurrences": int(nr.cost.kmer_occurrences)},
        "rekey_append_device_ms": stats(r_dev), "rekey_append_wall_ms": stats(r_wall),
        "union_preprocess_device_ms": stats(u_dev), "union_preprocess_wall_ms": stats(u_wall),
        "plain_append_device_ms": stats(p_dev), "plain_append_wall_ms": stats(p_wall),
        "stage_timers_on": {
            "rekey_ms": stats(rekey_ms), "merge_ms": stats(merge_ms), "rank_sort_ms": stats(rank_sort_ms), "rekey_bytes": rekey_bytes,
            "rekey_tb_per_s": rekey_bytes / (float(np.median(rekey_ms)) * 1e-3) / 1e12 if rekey_ms and np.median(rekey_ms) > 0 else None,
        },
    }
    r, u, p = out["rekey_append_device_ms"], out["union_preprocess_device_ms"], out["plain_append_device_ms"]
    out["device_ratio_median"] = r["median"] / u["median"]
    out["rekey_over_plain_append_median"] = r["median"] / p["median"]
    out["rekey_faster_ranges_apart"] = bool(r["median"] < u["median"] and r["p90"] < u["p10"])
    if check_genomes:
        fresh = PangeneNative.open()
        fresh.preprocess(k, *union_x)
        G = int(nr.cost.genomes)
        which = sorted(set(list(range(min(check_genomes - 1, G - 1))) + [G - 1]))
        ta, tb = nr.rank_table(), fresh.rank_table()
        same = nr.cost.as_dict() == fresh.cost.as_dict() and bool(np.array_equal(ta[0], tb[0])) and ta[1] == tb[1]
        da, db = score_digests(nr, which), score_digests(fresh, which)
        out["union_context_check"] = {"genomes": which, "verdict": "match" if same and da == db else "MISMATCH",
                                      "sha256_of_the_appended_genome": da[G - 1]}
        fresh.close()
    nr.close(); npl.close(); nu.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["mycoplasma64_standin", "synthetic_128x4000x300"])
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--split-repeat", type=int, default=5)
    ap.add_argument("--check-genomes", type=int, default=4, help="genomes whose Scores are compared with a union build (0: none)")
    ap.add_argument("--baseline-lib", default=None, help="libpandelos_amd.so of the parent commit (default: this library rebuilds)")
    ap.add_argument("--k", type=int, default=0, help="k-mer length instead of calculate_k's (a larger one gives 64-bit keys)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = []
    for c in args.config:
        r = measure(c, args.repeat, args.warmup, args.split_repeat, args.check_genomes, args.baseline_lib, args.k)
        res.append(r)
        print(json.dumps({kk: r.get(kk) for kk in ("config", "baseline", "device_ratio_median", "rekey_over_plain_append_median",
                                                   "rekey_faster_ranges_apart", "rekey_info")}), flush=True)
        print(json.dumps({kk: r[kk] for kk in ("rekey_append_device_ms", "union_preprocess_device_ms", "plain_append_device_ms", "stage_timers_on")}), flush=True)
        print(json.dumps(r.get("union_context_check", {})), flush=True)
        if args.out:                                    # (after every set: a long run keeps what it has)
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    return 1 if any(r.get("union_context_check", {}).get("verdict") == "MISMATCH" for r in res) else 0


if __name__ == "__main__":
    sys.exit(main())
