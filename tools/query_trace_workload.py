#!/usr/bin/env python3
"""The workload of a query's kernel trace: the query fixtures of tests/golden/query, each against its own base, once.

  single  one pdl_query_scores per fixture
  batch   one pdl_query_batch per fixture, of the fixture's query twice

Each block is checked against the fixture.  --root names the checkout whose library runs (default: this one), so the same
workload traces another build:

usage: rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/query_trace_workload.py single|batch
           [--root CHECKOUT] [--fixture wide_row_9000_columns protein_like_held_out]
"""
import argparse
import sys
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("single", "batch"))
ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]))
ap.add_argument("--fixture", nargs="+", default=["wide_row_9000_columns", "protein_like_held_out"])
args = ap.parse_args()
sys.path.insert(0, str(Path(args.root).resolve()))

from pandelos_amd.pangene_native import PangeneNative  # noqa: E402
from tests.test_query_golden import assert_block, load_case  # noqa: E402

for name in args.fixture:
    fx, base, query, k, G = load_case(name)
    nat = PangeneNative(k, base)
    if args.mode == "single":
        assert_block(nat.query_idata(query).as_dict(), fx, name)
    else:
        q = query.flatten()[:2]
        for block in nat.query_batch([q, q]):
            assert_block(block.as_dict(), fx, name)
    nat.close()
    print(f"{args.mode} {name}: equals the fixture", flush=True)
