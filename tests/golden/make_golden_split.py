#!/usr/bin/env python3
"""Regenerate tests/golden/split/*.net, *.faa and *.clus (build container only).

.net  = generated: the two-community components of tests/split_cases.py (a ring through all nodes plus random pairs, 3 % of them
        across the two halves, average degree about 9) with 100 and 200 nodes, and a network that holds both plus clean
        components (pairs of genes of two genomes)
.faa  = a dummy: one header per gene (16 genome labels dealt round-robin) and a one-letter sequence; only the headers are read
.clus = the reference's netclu_ng.py (with the installed networkx) run as a subprocess on (.faa, .net), followed by the text
        filter of pandelos.sh:79, as make_golden_net.py does
Only inputs/outputs are stored.
"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from tests.golden.make_golden_net import clus_of                 # noqa: E402
from tests.split_cases import two_community_edges                # noqa: E402

OUT = Path(__file__).resolve().parent / "split"
GENOMES = 16


def cases():
    e100, e200 = two_community_edges(100, 100), two_community_edges(200, 200)
    clean = [(300 + 2 * i, 301 + 2 * i) for i in range(30)]
    mixed = clean[:10] + e100 + clean[10:20] + [(a + 100, b + 100) for a, b in e200] + clean[20:]
    return {"community_100": (100, e100), "community_200": (200, e200), "community_mixed": (360, mixed)}


def main():
    OUT.mkdir(exist_ok=True)
    for name, (genes, edges) in cases().items():
        faa, net = OUT / f"{name}.faa", OUT / f"{name}.net"
        faa.write_text("".join(f"genome{g % GENOMES:02d}\tgene{g:04d}\tdummy\nM\n" for g in range(genes)))
        net.write_text("".join(f"{a}\t{b}\t1.0\n" for a, b in edges))
        clus = clus_of(faa, net)
        (OUT / f"{name}.clus").write_text(clus)
        fams = [l.split() for l in clus.splitlines()]
        print(name, "edges", len(edges), "families", len(fams), "genes", genes, "largest", max(len(f) for f in fams))


if __name__ == "__main__":
    main()
