#!/usr/bin/env python3
"""Time pdl_remove_genomes against the rebuild it replaces, on one GPU.

For a set of pandelos_amd.synth.CONFIGS one genome is held IN and then removed: the last one, and one from the middle.  Two
contexts in one process, "stage_timers" 0:
  remove   pdl_preprocess of the whole set (NOT timed), then timed: pdl_remove_genomes of the genome
           (wall time of the call and pdl_remove_info.device_ms)
  rebuild  timed: pdl_preprocess of the remaining set (wall time; device time = pdl_timings.preprocess_total_ms) — by the
           library given with --baseline-lib (a libpandelos_amd.so built from the parent commit in a side directory: not the
           library under test, although its preprocess path should be the same code), else by this library
Both leave the same context.  Warm-up first, then the two alternate --repeat times; median, min, max and the 10th / 90th
percentiles of each.  The stage split comes from --split-repeat further removals with "stage_timers" 1 (the event pairs around
the stages cost a few microseconds of idle stream each, so they stay out of the comparison).  The compaction's TB/s counts its
keys and gene values once in (M elements), the gene values once more for the count pass, and the kept ones once out:
(key bytes + 8) * M + (key bytes + 4) * M'.  compact_ms also holds the gene map and the zeroing of the control block.
After the timing the shrunk context with the genome appended again is checked against tests/golden/digests_baseline.json when
the set is pinned there (last genome only: the append puts it back where it was).

usage: python tools/remove_time.py [--config mycoplasma64_standin synthetic_128x4000x300] [--baseline-lib PATH] [--out FILE]
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
from tools.append_time import digests_match, stats  # noqa: E402


def open_with_library(path):
    """A PangeneNative whose calls go to another build of the library (only what this tool calls is declared)."""
    from pandelos_amd import _lib
    from pandelos_amd.pangene_native import PangeneNative
    _lib.load()                                         # (the HIP runtime this process uses is loaded first)
    lib = C.CDLL(str(path))
    vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
    lib.pdl_create.argtypes = [C.POINTER(_lib.PdlConfig)]; lib.pdl_create.restype = vp
    lib.pdl_destroy.argtypes = [vp]; lib.pdl_destroy.restype = None
    lib.pdl_last_error.argtypes = [vp]; lib.pdl_last_error.restype = C.c_char_p
    lib.pdl_preprocess.argtypes = [vp, vp, vp, vp, u32, i32, i32, C.POINTER(_lib.PdlCost)]; lib.pdl_preprocess.restype = i32
    lib.pdl_get_timings.argtypes = [vp, C.POINTER(_lib.PdlTimings)]; lib.pdl_get_timings.restype = i32
    lib.pdl_set_option.argtypes = [vp, C.c_char_p, C.c_int64]; lib.pdl_set_option.restype = i32
    nat = PangeneNative.__new__(PangeneNative)
    nat._lib = lib
    cfg = _lib.PdlConfig(device=-1, stream=None, flags=0, reserved=0)
    ctx = lib.pdl_create(C.byref(cfg))
    if not ctx:
        raise RuntimeError(f"{path}: pdl_create failed")
    nat._ctx = C.c_void_p(ctx)
    nat.cost = _lib.PdlCost()
    return nat


def measure(config: str, which: str, repeat: int, warmup: int, split_repeat: int, check: bool, baseline_lib) -> dict:
    from pandelos_amd.calculate_k import calculate_k
    from pandelos_amd.pangene_native import PangeneNative
    from pandelos_amd.remove import remaining_input
    from pandelos_amd.synth import CONFIGS, make_gene_set
    gs = make_gene_set(**CONFIGS[config])
    k = calculate_k(gs.residues)
    whole = (gs.residues, gs.offsets, gs.genome_of)
    G = int(gs.genome_of.max()) + 1
    g = G - 1 if which == "last" else G // 2
    rest = remaining_input(*whole, [g])
    nr = PangeneNative.open()
    nr.set_option("stage_timers", 0)
    nb = open_with_library(baseline_lib) if baseline_lib else PangeneNative.open()
    nb.set_option("stage_timers", 0)

    def run_remove():
        nr.preprocess(k, *whole)                        # the build of the whole set: outside the timed region
        t0 = time.perf_counter()
        nr.remove([g])
        return (time.perf_counter() - t0) * 1e3, nr.last_remove_info["device_ms"]

    def run_rebuild():
        t0 = time.perf_counter()
        nb.preprocess(k, *rest)
        return (time.perf_counter() - t0) * 1e3, nb.timings()["preprocess_total_ms"]

    for _ in range(warmup):
        run_remove()
        run_rebuild()
    r_wall, r_dev, b_wall, b_dev = [], [], [], []
    for _ in range(repeat):
        w, d = run_remove()
        r_wall.append(w); r_dev.append(d)
        w, d = run_rebuild()
        b_wall.append(w); b_dev.append(d)
    assert nr.cost.as_dict() == nb.cost.as_dict(), "the shrunk context and the rebuild disagree"
    info = dict(nr.last_remove_info)
    M1 = int(nr.cost.kmer_occurrences)
    M0 = M1 + int(info["kmer_occurrences"])
    key_bytes = 8 if nr.cost.rank_bits > 32 else 4
    compact_bytes = (key_bytes + 8) * M0 + (key_bytes + 4) * M1
    nr.set_option("stage_timers", 1)
    compact, stages = [], []
    for _ in range(split_repeat):
        run_remove()
        compact.append(nr.last_remove_info["compact_ms"])
        tm = nr.timings()
        stages.append({f: tm[f] for f in ("sort_rank_ms", "dict_ms", "sort_seq_ms", "ranges_ms", "preprocess_total_ms")})
    nb.set_option("stage_timers", 1)
    nb.preprocess(k, *rest)
    tb = nb.timings()
    out = {
        "config": config, "shape": CONFIGS[config], "k": k, "removed_genome": g, "which": which,
        "baseline": "parent commit's library" if baseline_lib else "this library",
        "whole": {"sequences": int(len(gs.genome_of)), "genomes": G, "kmer_occurrences": M0, "key_bytes": key_bytes},
        "removed": {kk: info[kk] for kk in ("sequences", "residues", "kmer_occurrences", "records")},
        "remove_device_ms": stats(r_dev), "remove_wall_ms": stats(r_wall),
        "rebuild_preprocess_device_ms": stats(b_dev), "rebuild_preprocess_wall_ms": stats(b_wall),
        "stage_timers_on": {
            "compact_ms": stats(compact), "compact_bytes": compact_bytes,
            "compact_tb_per_s": compact_bytes / (float(np.median(compact)) * 1e-3) / 1e12 if compact and np.median(compact) > 0 else None,
            "remove_stage_ms_median": {f: float(np.median([s[f] for s in stages])) for f in stages[0]} if stages else {},
            "rebuild_preprocess_stage_ms": {f: tb[f] for f in ("hist_ms", "rank_ms", "sort_rank_ms", "dict_ms", "sort_seq_ms", "ranges_ms", "preprocess_total_ms")},
        },
    }
    a, u = out["remove_device_ms"], out["rebuild_preprocess_device_ms"]
    out["device_ratio_median"] = a["median"] / u["median"]
    out["wall_ratio_median"] = out["remove_wall_ms"]["median"] / out["rebuild_preprocess_wall_ms"]["median"]
    out["remove_faster_ranges_apart"] = bool(a["median"] < u["median"] and a["p90"] < u["p10"])
    if check:
        pinned = json.loads((ROOT / "tests" / "golden" / "digests_baseline.json").read_text())
        if config in pinned and which == "last":
            n = int((gs.genome_of != g).sum())
            nr.append(gs.residues[int(gs.offsets[n]):], gs.offsets[n:] - gs.offsets[n])
            out["reference_digests"] = "match" if digests_match(nr, pinned[config]) else "MISMATCH"
        else:
            out["reference_digests"] = "not pinned"
    nr.close(); nb.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["mycoplasma64_standin", "synthetic_128x4000x300"])
    ap.add_argument("--which", nargs="+", default=["last", "middle"], choices=["last", "middle"])
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--split-repeat", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None, help="libpandelos_amd.so of the parent commit (default: this library rebuilds)")
    ap.add_argument("--no-check", action="store_true", help="skip the digest check")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = []
    for c in args.config:
        for which in args.which:
            r = measure(c, which, args.repeat, args.warmup, args.split_repeat, not args.no_check, args.baseline_lib)
            res.append(r)
            print(json.dumps({kk: r.get(kk) for kk in ("config", "which", "baseline", "device_ratio_median", "wall_ratio_median",
                                                       "remove_faster_ranges_apart", "reference_digests")}), flush=True)
            print(json.dumps({"remove_device_ms": r["remove_device_ms"], "rebuild_preprocess_device_ms": r["rebuild_preprocess_device_ms"],
                              "stage_timers_on": r["stage_timers_on"]}), flush=True)
            if args.out:                                # (after every measurement: a long run keeps what it has)
                Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    return 1 if any(r.get("reference_digests") == "MISMATCH" for r in res) else 0


if __name__ == "__main__":
    sys.exit(main())
