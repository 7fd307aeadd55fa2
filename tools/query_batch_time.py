#!/usr/bin/env python3
"""Time pdl_query_batch against the consecutive pdl_query_scores calls it replaces, on one GPU and in one process.

For a set of pandelos_amd.synth.CONFIGS the last q genomes are held out as q independent queries; the base is the rest.
Two contexts on the same base, "stage_timers" 0:
  batch       timed: ONE pdl_query_batch of the q genomes and the freeing of its blocks (wall time of the C calls, and
              pdl_query_batch_info.device_ms)
  sequential  timed: q pdl_query_scores calls, one per genome, each block freed (wall time, and the sum of their device_ms) —
              by the library given with --baseline-lib (a libpandelos_amd.so built from the parent commit in a side directory),
              else by this library
Both go through ctypes straight to the C ABI: no block is copied into numpy inside the timed region.  Warm-up first, then the two
alternate --repeat times; median, min, max and the 10th / 90th percentiles of each.  Once per measurement the batch's blocks
are compared byte for byte with the sequential ones.  For the ratio DESIGN.md §9 uses, the union rebuild (pdl_preprocess +
pdl_score_all of base + the first held-out genome, this library) is timed --union-repeat times.

With --rekey-copies N (default 0: off) the batch is instead N copies of tools/query_rekey_time.py's genome — the last genome of
CONFIG with ONE residue replaced by a letter the set lacks — against the other genomes, option "query_rekey" on in both contexts:
a re-keyed chunk.  No union rebuild is timed then.

usage: python tools/query_batch_time.py [--config mycoplasma64_standin:8 mycoplasma64_standin:32 synthetic_128x4000x300:8]
                                        [--rekey-copies N] [--baseline-lib PATH] [--out FILE]
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
from tools.query_time import stats  # noqa: E402

BLOCK_ARRAYS = (("scores", 4, "z"), ("percs", 4, "z"), ("tr_percs", 4, "z"), ("row", 4, "z"), ("column", 4, "z"), ("first_seq_genome", 4, "z"),
                ("second_seq_genome", 4, "z"), ("max_genome_score", 4, "m"), ("max_genome_score_col", 4, "n"), ("scoresMaxMappings", 4, "n"))


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
    lib.pdl_query_scores.argtypes = [vp, vp, vp, u32, C.POINTER(_lib.PdlScores), C.POINTER(_lib.PdlQueryInfo)]; lib.pdl_query_scores.restype = i32
    lib.pdl_free_scores.argtypes = [C.POINTER(_lib.PdlScores)]; lib.pdl_free_scores.restype = None
    nat = PangeneNative.__new__(PangeneNative)
    nat._lib = lib
    cfg = _lib.PdlConfig(device=-1, stream=None, flags=0, reserved=0)
    ctx = lib.pdl_create(C.byref(cfg))
    if not ctx:
        raise RuntimeError(f"{path}: pdl_create failed")
    nat._ctx = C.c_void_p(ctx)
    nat.cost = _lib.PdlCost()
    return nat


def block_bytes(s) -> bytes:
    """Every array of a pdl_scores block, for the byte-for-byte comparison."""
    count = {"z": s.scoresCount, "m": s.rows * s.genomes, "n": s.sequences}
    head = np.array([s.scoresCount, s.rows, s.genomes, s.sequences], np.uint32).tobytes()
    return head + b"".join(C.string_at(getattr(s, f), w * count[c]) if count[c] else b"" for f, w, c in BLOCK_ARRAYS)


def split_last_genomes(gs, q):
    """(base arrays, [query arrays], union of the base and the first query); synth sets are genome major."""
    G = int(gs.genome_of.max()) + 1
    off = gs.offsets.astype(np.int64)

    def cut(sel):
        idx = np.flatnonzero(sel)
        lo, hi = int(off[idx[0]]), int(off[idx[-1] + 1])
        return gs.residues[lo:hi].copy(), (off[idx[0]:idx[-1] + 2] - lo).astype(np.uint64)
    rb, ob_ = cut(gs.genome_of < G - q)
    gb = gs.genome_of[gs.genome_of < G - q].astype(np.uint32)
    queries = [cut(gs.genome_of == g) for g in range(G - q, G)]
    rq, oq = queries[0]
    union = (np.concatenate([rb, rq]), np.concatenate([ob_, ob_[-1] + oq[1:]]).astype(np.uint64),
             np.concatenate([gb, np.full(len(oq) - 1, G - q, np.uint32)]))
    return (rb, ob_, gb), queries, union


def letter_bearing_copies(gs, k, copies):
    """(base arrays, `copies` times the last genome with a letter the set lacks in the middle of its first gene that has a k-mer)"""
    from tools.query_time import split_last_genome
    base, query, _ = split_last_genome(gs)
    present = np.zeros(256, bool)
    present[gs.residues] = True
    letter = next(b for b in b"XUBZOJ*" if not present[b])
    qx = query[0].copy()
    lens = np.diff(query[1].astype(np.int64))
    gene = int(np.argmax(lens >= k))
    qx[int(query[1][gene]) + int(lens[gene]) // 2] = letter
    return base, [(qx, query[1])] * copies


def measure(config: str, q: int, repeat: int, warmup: int, union_repeat: int, baseline_lib, rekey_copies: int = 0) -> dict:
    from pandelos_amd import _lib
    from pandelos_amd.calculate_k import calculate_k
    from pandelos_amd.pangene_native import PangeneNative
    from pandelos_amd.synth import CONFIGS, make_gene_set
    gs = make_gene_set(**CONFIGS[config])
    k = calculate_k(gs.residues)
    if rekey_copies:
        q, union_repeat = rekey_copies, -1
        base, queries = letter_bearing_copies(gs, k, q)
    else:
        base, queries, union = split_last_genomes(gs, q)
    nb = PangeneNative.open()
    ns = open_with_library(baseline_lib) if baseline_lib else PangeneNative.open()
    for nat in (nb, ns):
        nat.set_option("stage_timers", 0)
        if rekey_copies:
            nat.set_option("query_rekey", 1)
        nat.preprocess(k, *base)
    res, off, begin = PangeneNative.pack_queries(queries)
    n = len(off) - 1
    blocks, infos, binfo = (_lib.PdlScores * q)(), (_lib.PdlQueryInfo * q)(), _lib.PdlQueryBatchInfo()
    singles = [(np.ascontiguousarray(r), np.ascontiguousarray(o), _lib.PdlScores(), _lib.PdlQueryInfo()) for r, o in queries]

    def run_batch(keep=None):
        t0 = time.perf_counter()
        rc = nb._lib.pdl_query_batch(nb._ctx, res.ctypes.data, off.ctypes.data, begin.ctypes.data, n, q, blocks, infos, C.byref(binfo))
        t1 = time.perf_counter()
        nb._check(rc)
        if keep is not None:
            keep.extend(block_bytes(blocks[j]) for j in range(q))
        t2 = time.perf_counter()
        for j in range(q):
            nb._lib.pdl_free_scores(C.byref(blocks[j]))
        return (t1 - t0 + time.perf_counter() - t2) * 1e3, binfo.device_ms

    def run_sequential(keep=None):
        wall, dev = 0.0, 0.0
        for r, o, s, info in singles:
            t0 = time.perf_counter()
            rc = ns._lib.pdl_query_scores(ns._ctx, r.ctypes.data, o.ctypes.data, len(o) - 1, C.byref(s), C.byref(info))
            t1 = time.perf_counter()
            ns._check(rc)
            if keep is not None:
                keep.append(block_bytes(s))
            t2 = time.perf_counter()
            ns._lib.pdl_free_scores(C.byref(s))
            wall += t1 - t0 + time.perf_counter() - t2
            dev += info.device_ms
        return wall * 1e3, dev

    a, b = [], []
    run_batch(a)
    run_sequential(b)
    equal = a == b
    cells = sum(int(np.frombuffer(x[:4], np.uint32)[0]) for x in a)
    for _ in range(warmup):
        run_batch()
        run_sequential()
    b_wall, b_dev, s_wall, s_dev = [], [], [], []
    for _ in range(repeat):
        w, d = run_batch()
        b_wall.append(w); b_dev.append(d)
        w, d = run_sequential()
        s_wall.append(w); s_dev.append(d)
    chunks = int(binfo.chunks)
    nu = PangeneNative.open()
    nu.set_option("stage_timers", 0)
    u_dev = []
    for _ in range(union_repeat + 1):
        nu.preprocess(k, *union)
        nu.score_all()
        tm = nu.timings()
        u_dev.append(tm["preprocess_total_ms"] + tm["score_total_ms"])
    u_dev = u_dev[1:]
    out = {
        "config": config, "shape": CONFIGS[config], "k": k, "queries": q, "chunks": chunks, "rekeyed_copies_of_one_genome": bool(rekey_copies),
        "baseline": "parent commit's library" if baseline_lib else "this library",
        "base": {"sequences": int(nb.cost.sequences), "genomes": int(nb.cost.genomes), "records": int(nb.cost.dictionary_records)},
        "batch": {"genes": n, "residues": int(off[-1]), "cells": cells},
        "blocks_equal_the_sequential_ones": bool(equal),
        "batch_device_ms": stats(b_dev), "batch_wall_ms": stats(b_wall),
        "sequential_device_ms": stats(s_dev), "sequential_wall_ms": stats(s_wall),
        "union_rebuild_device_ms": stats(u_dev) if u_dev else None,
    }
    out["per_query_device_ms"] = {"batch": out["batch_device_ms"]["median"] / q, "sequential": out["sequential_device_ms"]["median"] / q}
    out["per_query_wall_ms"] = {"batch": out["batch_wall_ms"]["median"] / q, "sequential": out["sequential_wall_ms"]["median"] / q}
    out["device_speedup_median"] = out["sequential_device_ms"]["median"] / out["batch_device_ms"]["median"]
    out["wall_speedup_median"] = out["sequential_wall_ms"]["median"] / out["batch_wall_ms"]["median"]
    out["batch_faster_ranges_apart"] = {"device": bool(out["batch_device_ms"]["p90"] < out["sequential_device_ms"]["p10"]),
                                        "wall": bool(out["batch_wall_ms"]["p90"] < out["sequential_wall_ms"]["p10"])}
    if u_dev:
        u = out["union_rebuild_device_ms"]["median"]
        out["per_query_ratio_to_union_rebuild"] = {"batch": out["per_query_device_ms"]["batch"] / u, "sequential": out["per_query_device_ms"]["sequential"] / u}
        out["target_quarter_met"] = bool(out["per_query_ratio_to_union_rebuild"]["batch"] <= 0.25)
    nb.close(); ns.close(); nu.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["mycoplasma64_standin:8", "mycoplasma64_standin:32", "synthetic_128x4000x300:8"],
                    help="CONFIG:Q — the last Q genomes of CONFIG are the queries")
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--union-repeat", type=int, default=5)
    ap.add_argument("--rekey-copies", type=int, default=0, help="N > 0: the batch is N copies of the last genome with a letter the set lacks, query_rekey on")
    ap.add_argument("--baseline-lib", default=None, help="libpandelos_amd.so of the parent commit (default: this library's pdl_query_scores)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = []
    for spec in args.config:
        config, _, q = spec.partition(":")
        r = measure(config, int(q or 8), args.repeat, args.warmup, args.union_repeat, args.baseline_lib, args.rekey_copies)
        res.append(r)
        print(json.dumps({kk: r.get(kk) for kk in ("config", "queries", "chunks", "baseline", "blocks_equal_the_sequential_ones", "device_speedup_median",
                                                   "wall_speedup_median", "batch_faster_ranges_apart", "per_query_device_ms",
                                                   "per_query_ratio_to_union_rebuild", "target_quarter_met")}), flush=True)
        print(json.dumps({kk: r[kk] for kk in ("batch_device_ms", "sequential_device_ms", "batch_wall_ms", "sequential_wall_ms")}), flush=True)
        if args.out:                                    # (after every measurement: a long run keeps what it has)
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0 if all(r["blocks_equal_the_sequential_ones"] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
