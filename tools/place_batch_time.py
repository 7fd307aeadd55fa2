#!/usr/bin/env python3
"""Time pdl_place_batch against the consecutive pdl_place_query calls it replaces, on one GPU and in one process.

For a set of pandelos_amd.synth.CONFIGS the last q genomes are held out as q independent queries; the base is the rest.
Contexts on the same base, "stage_timers" 0, families computed before anything is timed:
  batch            timed: ONE pdl_place_batch of the q genomes and the freeing of its placements (wall time of the C calls, and
                   pdl_place_batch_info.device_ms) — this library
  sequential       timed: q pdl_place_query calls, one per genome, each placement freed (wall time, and the sum of their
                   device_ms) — by the library given with --baseline-lib (a libpandelos_amd.so built from the parent commit in
                   a side directory)
  sequential_this  the same q calls by this library (with --baseline-lib; without it `sequential` is this library's)
All go through ctypes straight to the C ABI: no placement is copied into numpy inside the timed region.  Warm-up first, then the
variants alternate --repeat times; median, min, max and the 10th / 90th percentiles of each.  In EVERY round the batch's
placements are compared byte for byte (every field but device_ms) with the sequential ones of that round, outside the timed
regions; a difference ends the run with an error.

usage: python tools/place_batch_time.py [--config mycoplasma64_standin:8 mycoplasma64_standin:32 synthetic_128x4000x300:8]
                                        [--baseline-lib PATH] [--out FILE]
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
from tools.query_batch_time import split_last_genomes  # noqa: E402
from tools.query_time import stats  # noqa: E402

COUNTS = ("sequences", "n_query", "genomes", "edges", "edges_phase1", "groups", "novel", "joined", "bridging", "colliding", "unplaced")


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
    lib.pdl_set_option.argtypes = [vp, C.c_char_p, C.c_int64]; lib.pdl_set_option.restype = i32
    lib.pdl_place_query.argtypes = [vp, vp, vp, u32, C.POINTER(_lib.PdlPlacement), C.POINTER(_lib.PdlQueryInfo)]; lib.pdl_place_query.restype = i32
    lib.pdl_free_placement.argtypes = [C.POINTER(_lib.PdlPlacement)]; lib.pdl_free_placement.restype = None
    nat = PangeneNative.__new__(PangeneNative)
    nat._lib = lib
    cfg = _lib.PdlConfig(device=-1, stream=None, flags=0, reserved=0)
    ctx = lib.pdl_create(C.byref(cfg))
    if not ctx:
        raise RuntimeError(f"{path}: pdl_create failed")
    nat._ctx = C.c_void_p(ctx)
    nat.cost = _lib.PdlCost()
    return nat


def placement_bytes(p) -> bytes:
    """Every field of a pdl_placement but device_ms, for the byte-for-byte comparison."""
    head = np.array([getattr(p, f) for f in COUNTS], np.uint32).tobytes()
    grab = lambda ptr, nbytes: C.string_at(ptr, nbytes) if nbytes else b""
    g, n, e = p.groups, p.n_query, p.edges
    q_off, b_off = grab(p.group_query_off, 4 * (g + 1)), grab(p.group_base_off, 4 * (g + 1))
    nodes, pairs = (int(np.frombuffer(x, np.uint32)[-1]) for x in (q_off, b_off))
    return head + b"".join([grab(p.src, 4 * e), grab(p.dst, 4 * e), grab(p.score, 4 * e), grab(p.family_of, 4 * n), grab(p.is_node, n),
                            grab(p.group_label, 4 * g), q_off, grab(p.group_query, 4 * nodes), b_off, grab(p.group_base, 4 * pairs),
                            grab(p.group_collides, g)])


def measure(config: str, q: int, repeat: int, warmup: int, baseline_lib) -> dict:
    from pandelos_amd import _lib
    from pandelos_amd.calculate_k import calculate_k
    from pandelos_amd.pangene_native import PangeneNative
    from pandelos_amd.synth import CONFIGS, make_gene_set
    gs = make_gene_set(**CONFIGS[config])
    k = calculate_k(gs.residues)
    base, queries, _ = split_last_genomes(gs, q)
    nb = PangeneNative.open()
    seq = {"sequential": open_with_library(baseline_lib) if baseline_lib else PangeneNative.open()}
    if baseline_lib:
        seq["sequential_this"] = PangeneNative.open()
    for nat in (nb, *seq.values()):
        nat.set_option("stage_timers", 0)
        nat.preprocess(k, *base)
    res, off, begin = PangeneNative.pack_queries(queries)
    n = len(off) - 1
    pls, infos, binfo = (_lib.PdlPlacement * q)(), (_lib.PdlQueryInfo * q)(), _lib.PdlPlaceBatchInfo()
    singles = [(np.ascontiguousarray(r), np.ascontiguousarray(o), _lib.PdlPlacement(), _lib.PdlQueryInfo()) for r, o in queries]

    def run_batch(keep):
        t0 = time.perf_counter()
        rc = nb._lib.pdl_place_batch(nb._ctx, res.ctypes.data, off.ctypes.data, begin.ctypes.data, n, q, pls, infos, C.byref(binfo))
        t1 = time.perf_counter()
        nb._check(rc)
        keep.extend(placement_bytes(pls[j]) for j in range(q))
        t2 = time.perf_counter()
        for j in range(q):
            nb._lib.pdl_free_placement(C.byref(pls[j]))
        return (t1 - t0 + time.perf_counter() - t2) * 1e3, binfo.device_ms

    def run_sequential(ns, keep):
        wall, dev = 0.0, 0.0
        for r, o, p, info in singles:
            t0 = time.perf_counter()
            rc = ns._lib.pdl_place_query(ns._ctx, r.ctypes.data, o.ctypes.data, len(o) - 1, C.byref(p), C.byref(info))
            t1 = time.perf_counter()
            ns._check(rc)
            dev += p.device_ms
            keep.append(placement_bytes(p))
            t2 = time.perf_counter()
            ns._lib.pdl_free_placement(C.byref(p))
            wall += t1 - t0 + time.perf_counter() - t2
        return wall * 1e3, dev

    def one_round(times):
        a = []
        w, d = run_batch(a)
        if times is not None:
            times["batch"][0].append(w); times["batch"][1].append(d)
        for name, ns in seq.items():
            b = []
            w, d = run_sequential(ns, b)
            if a != b:
                raise SystemExit(f"{config}:{q}: the batch's placements differ from the {name} ones")
            if times is not None:
                times[name][0].append(w); times[name][1].append(d)
        return a

    first = one_round(None)                                 # (the families are computed here, on first use)
    edges = sum(int(np.frombuffer(x[12:16], np.uint32)[0]) for x in first)
    groups = sum(int(np.frombuffer(x[20:24], np.uint32)[0]) for x in first)
    for _ in range(warmup):
        one_round(None)
    times = {name: ([], []) for name in ("batch", *seq)}
    for _ in range(repeat):
        one_round(times)
    out = {
        "config": config, "shape": CONFIGS[config], "k": k, "queries": q, "chunks": int(binfo.chunks),
        "baseline": "parent commit's library" if baseline_lib else "this library",
        "base": {"sequences": int(nb.cost.sequences), "genomes": int(nb.cost.genomes), "records": int(nb.cost.dictionary_records)},
        "batch": {"genes": n, "residues": int(off[-1]), "edges": edges, "groups": groups},
        "placements_equal_the_sequential_ones_in_every_round": True,
    }
    for name, (wall, dev) in times.items():
        out[f"{name}_device_ms"] = stats(dev); out[f"{name}_wall_ms"] = stats(wall)
    out["per_query_device_ms"] = {name: out[f"{name}_device_ms"]["median"] / q for name in times}
    out["per_query_wall_ms"] = {name: out[f"{name}_wall_ms"]["median"] / q for name in times}
    out["device_speedup_median"] = out["sequential_device_ms"]["median"] / out["batch_device_ms"]["median"]
    out["wall_speedup_median"] = out["sequential_wall_ms"]["median"] / out["batch_wall_ms"]["median"]
    out["batch_faster_ranges_apart"] = {"device": bool(out["batch_device_ms"]["p90"] < out["sequential_device_ms"]["p10"]),
                                        "wall": bool(out["batch_wall_ms"]["p90"] < out["sequential_wall_ms"]["p10"])}
    if baseline_lib:                                        # the refactor's own bar: this build's sequential median not above the parent's p90
        out["sequential_this_not_above_parent_p90"] = {"device": bool(out["sequential_this_device_ms"]["median"] <= out["sequential_device_ms"]["p90"]),
                                                       "wall": bool(out["sequential_this_wall_ms"]["median"] <= out["sequential_wall_ms"]["p90"])}
    nb.close()
    for ns in seq.values():
        ns.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["mycoplasma64_standin:8", "mycoplasma64_standin:32", "synthetic_128x4000x300:8"],
                    help="CONFIG:Q — the last Q genomes of CONFIG are the queries")
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None, help="libpandelos_amd.so of the parent commit (default: this library's pdl_place_query)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = []
    for spec in args.config:
        config, _, q = spec.partition(":")
        r = measure(config, int(q or 8), args.repeat, args.warmup, args.baseline_lib)
        res.append(r)
        print(json.dumps({kk: r.get(kk) for kk in ("config", "queries", "chunks", "baseline", "device_speedup_median", "wall_speedup_median",
                                                   "batch_faster_ranges_apart", "sequential_this_not_above_parent_p90", "per_query_device_ms",
                                                   "per_query_wall_ms")}), flush=True)
        print(json.dumps({kk: r[kk] for kk in r if kk.endswith("_device_ms") or kk.endswith("_wall_ms")}), flush=True)
        if args.out:                                    # (after every measurement: a long run keeps what it has)
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
