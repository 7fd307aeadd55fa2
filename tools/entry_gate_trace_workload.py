#!/usr/bin/env python3
"""The workloads of the kernel traces that compare the build, score and multi-GPU entry points of two builds of the library
(profiles/entry_gate_sequences.json), on the small set of tests/test_gpu_build_entry_refusals.py (4 genomes x 12 genes, k = 3):

  device   pdl_preprocess_device + pdl_score_all + every Scores block
  ingest   the same set written as a .faa file: pdl_ingest_faa + pdl_preprocess_ingested + pdl_score_all + every block
  dist2    a two-rank multi-GPU build and pass on one device (LocalRanks(2)) + every block from its owner
  query    a built context and one pdl_query_scores of the last genome's genes

Every block is compared with the CPU oracle.  --root names the checkout whose library runs (default: this one), so the same
workload traces another build:

usage: rocprofv3 --kernel-trace -d DIR --output-format csv -- python tools/entry_gate_trace_workload.py MODE [--root CHECKOUT]
"""
import argparse
import sys
import tempfile
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("device", "ingest", "dist2", "query"))
ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]))
args = ap.parse_args()
sys.path.insert(0, str(Path(args.root).resolve()))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from oracle import binding as ob  # noqa: E402
from pandelos_amd.distributed import LocalRanks  # noqa: E402
from pandelos_amd.pangene_native import PangeneNative  # noqa: E402
from pandelos_amd.synth import make_gene_set  # noqa: E402
from tests import helpers as H  # noqa: E402

K = 3
gs = make_gene_set(genomes=4, genes_per_genome=12, mean_len=40, sub_rate=0.1, seed=11)
ora = ob.Oracle(gs.residues, gs.offsets, gs.genome_of, K)
dev = torch.device("cuda", 0)
t_res = torch.from_numpy(np.concatenate([gs.residues, np.zeros((-len(gs.residues)) % 16 + 16, np.uint8)])).to(dev)
t_off = torch.from_numpy(gs.offsets.astype(np.int64)).to(dev)
t_gen = torch.from_numpy(gs.genome_of.astype(np.int32)).to(dev)


def check(block_of):
    for g in range(gs.genomes):
        H.assert_scores_equal(block_of(g).as_dict(), ora.scores(g), f"{args.mode}: genome {g}")


if args.mode == "dist2":
    ranks = LocalRanks(2)
    ranks.preprocess(K, t_res, t_off, t_gen, gs.genes, len(gs.residues))
    ranks.score_all()
    check(ranks.generate_scores_part)
    ranks.close()
else:
    nat = PangeneNative.open()
    if args.mode == "ingest":
        with tempfile.TemporaryDirectory() as d:
            gs.write_faa(Path(d) / "set.faa")
            nat.ingest_faa(Path(d) / "set.faa")
        nat.preprocess_ingested(K)
    elif args.mode == "device":
        nat.preprocess_device(K, t_res.data_ptr(), t_off.data_ptr(), t_gen.data_ptr(), gs.genes, len(gs.residues), keepalive=(t_res, t_off, t_gen))
    else:
        nat.preprocess(K, gs.residues, gs.offsets, gs.genome_of)
    if args.mode == "query":
        ids = np.nonzero(gs.genome_of == gs.genomes - 1)[0]
        lo, hi = int(gs.offsets[ids[0]]), int(gs.offsets[ids[-1] + 1])
        nat.query_scores(gs.residues[lo:hi].copy(), (gs.offsets[ids[0]:ids[-1] + 2] - np.uint64(lo)).astype(np.uint64))
    else:
        nat.score_all()
        check(nat.generate_scores_part)
    nat.close()
print(f"{args.mode}: done" if args.mode == "query" else f"{args.mode}: equals the oracle", flush=True)
