#!/usr/bin/env python3
"""Time pdl_append_genomes against the rebuild it replaces, on one GPU.

For a set of pandelos_amd.synth.CONFIGS the last genome is held out.  Two contexts in one process, "stage_timers" 0:
  append  pdl_preprocess of the other G-1 genomes (NOT timed), then timed: pdl_append_genomes of the held-out genome
          (wall time of the call and pdl_append_info.device_ms)
  union   timed: pdl_preprocess of the whole set (wall time; device time = pdl_timings.preprocess_total_ms)
Both leave the same context.  Warm-up first, then the two alternate --repeat times; median, min, max and the 10th / 90th
percentiles of each.  The stage split (rank_sort_ms, merge_ms, the tail) comes from --split-repeat further appends with
"stage_timers" 1 — the event pairs around the stages cost a few microseconds of idle stream each, so they stay out of the
comparison; the merge's GB/s counts its keys and gene values once in, once out: 2 * (key bytes + 4) * (M + m).
After the timing the appended context is checked against tests/golden/digests_baseline.json when the set is pinned there.

usage: python tools/append_time.py [--config mycoplasma64_standin synthetic_128x4000x300] [--repeat 20] [--out FILE]
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
FIELDS = ("scores", "percs", "tr_percs", "row", "column", "first_seq_genome", "second_seq_genome",
          "max_genome_score", "max_genome_score_col", "scoresMaxMappings")


def stats(xs):
    a = np.asarray(xs, np.float64)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()),
            "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90)), "n": int(len(a))}


def split_last_genome(gs):
    """(base arrays, new genome's arrays): make_gene_set lays the genomes out one after the other."""
    held = int(gs.genome_of.max())
    n = int((gs.genome_of != held).sum())
    assert (gs.genome_of[:n] != held).all()
    cut = int(gs.offsets[n])
    return (gs.residues[:cut], gs.offsets[:n + 1], gs.genome_of[:n]), (gs.residues[cut:], gs.offsets[n:] - gs.offsets[n])


def digests_match(nat, d) -> bool:
    if nat.cost.total_cost != d["total_cost"]:
        return False
    for g in range(d["genomes"]):
        s = nat.generate_scores_part(g).as_dict()
        if int(s["scoresCount"]) != d["scoresCount"][g]:
            return False
        for f in FIELDS:
            a = np.ascontiguousarray(s[f])
            a = a.view(np.uint32) if a.dtype == np.float32 else a
            if hashlib.sha256(a.tobytes()).hexdigest() != d["sha256"][g][f]:
                return False
    return True


def measure(config: str, repeat: int, warmup: int, split_repeat: int, check: bool) -> dict:
    from pandelos_amd.calculate_k import calculate_k
    from pandelos_amd.pangene_native import PangeneNative
    from pandelos_amd.synth import CONFIGS, make_gene_set
    gs = make_gene_set(**CONFIGS[config])
    k = calculate_k(gs.residues)
    base, new = split_last_genome(gs)
    union = (gs.residues, gs.offsets, gs.genome_of)
    na = PangeneNative.open()
    na.set_option("stage_timers", 0)
    nu = PangeneNative.open()
    nu.set_option("stage_timers", 0)

    def run_append():
        na.preprocess(k, *base)                         # the base build: outside the timed region
        t0 = time.perf_counter()
        na.append(*new)
        return (time.perf_counter() - t0) * 1e3, na.last_append_info["device_ms"]

    def run_union():
        t0 = time.perf_counter()
        nu.preprocess(k, *union)
        return (time.perf_counter() - t0) * 1e3, nu.timings()["preprocess_total_ms"]

    for _ in range(warmup):
        run_append()
        run_union()
    a_wall, a_dev, u_wall, u_dev = [], [], [], []
    for _ in range(repeat):
        w, d = run_append()
        a_wall.append(w); a_dev.append(d)
        w, d = run_union()
        u_wall.append(w); u_dev.append(d)
    assert na.cost.as_dict() == nu.cost.as_dict(), "the appended context and the union build disagree"
    M, m = int(nu.cost.kmer_occurrences), int(na.last_append_info["kmer_occurrences"])
    key_bytes = 8 if nu.cost.rank_bits > 32 else 4
    merge_bytes = 2 * (key_bytes + 4) * M
    # the stage split, with the stage timers on
    na.set_option("stage_timers", 1)
    rank_sort, merge, stages = [], [], []
    for _ in range(split_repeat):
        run_append()
        info = na.last_append_info
        rank_sort.append(info["rank_sort_ms"]); merge.append(info["merge_ms"])
        tm = na.timings()
        stages.append({f: tm[f] for f in ("rank_ms", "sort_rank_ms", "dict_ms", "sort_seq_ms", "ranges_ms", "preprocess_total_ms")})
    nu.set_option("stage_timers", 1)
    nu.preprocess(k, *union)
    tu = nu.timings()
    out = {
        "config": config, "shape": CONFIGS[config], "k": k,
        "base": {"sequences": int(len(base[2])), "genomes": int(base[2].max()) + 1},
        "new_genome": {"genes": int(len(new[1]) - 1), **{kk: na.last_append_info[kk] for kk in ("residues", "kmer_occurrences", "records")}},
        "union": {"sequences": int(nu.cost.sequences), "kmer_occurrences": M, "records": int(nu.cost.dictionary_records), "key_bytes": key_bytes},
        "append_device_ms": stats(a_dev), "append_wall_ms": stats(a_wall),
        "union_preprocess_device_ms": stats(u_dev), "union_preprocess_wall_ms": stats(u_wall),
        "stage_timers_on": {
            "rank_sort_ms": stats(rank_sort), "merge_ms": stats(merge),
            "merge_bytes": merge_bytes, "merge_gb_per_s": merge_bytes / (float(np.median(merge)) * 1e-3) / 1e9 if merge and np.median(merge) > 0 else None,
            "append_stage_ms_median": {f: float(np.median([s[f] for s in stages])) for f in stages[0]} if stages else {},
            "union_preprocess_stage_ms": {f: tu[f] for f in ("hist_ms", "rank_ms", "sort_rank_ms", "dict_ms", "sort_seq_ms", "ranges_ms", "preprocess_total_ms")},
        },
    }
    a, u = out["append_device_ms"], out["union_preprocess_device_ms"]
    out["device_ratio_median"] = a["median"] / u["median"]
    out["wall_ratio_median"] = out["append_wall_ms"]["median"] / out["union_preprocess_wall_ms"]["median"]
    out["append_faster_ranges_apart"] = bool(a["median"] < u["median"] and a["p90"] < u["p10"])
    if check:
        pinned = json.loads((ROOT / "tests" / "golden" / "digests_baseline.json").read_text())
        out["reference_digests"] = ("match" if digests_match(na, pinned[config]) else "MISMATCH") if config in pinned else "not pinned"
    na.close(); nu.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["mycoplasma64_standin", "synthetic_128x4000x300"])
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--split-repeat", type=int, default=5)
    ap.add_argument("--no-check", action="store_true", help="skip the digest check of the appended context")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = []
    for c in args.config:
        r = measure(c, args.repeat, args.warmup, args.split_repeat, not args.no_check)
        res.append(r)
        print(json.dumps({kk: r.get(kk) for kk in ("config", "device_ratio_median", "wall_ratio_median", "append_faster_ranges_apart", "reference_digests")}), flush=True)
        print(json.dumps({"append_device_ms": r["append_device_ms"], "union_preprocess_device_ms": r["union_preprocess_device_ms"],
                          "stage_timers_on": r["stage_timers_on"]}), flush=True)
        if args.out:                                    # (after every set: a long run keeps what it has)
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    return 1 if any(r.get("reference_digests") == "MISMATCH" for r in res) else 0


if __name__ == "__main__":
    sys.exit(main())
