"""Place one newly sequenced genome into a pan-genome's gene families without committing it.

    python -m pandelos_amd.place -i base.faa -k K -q new.faa -o new.tsv [--net new.net] [--rekey]

The base set is ingested, its dictionary built and its families clustered once on the device; the query file (one genome, read
like ``PangeneIData.readFromFile``) is scored against the dictionary, its block is filtered to the edges its own task adds to the
network, and those edges are hung onto the base network's components — all in HBM (``pdl_place_query``).  The base is only read.

``new.tsv`` holds one line per query gene, tab-separated:

    gene  status  representative  fused_base_families  collides

status is ``unplaced`` (no edge), ``novel`` (a family of query genes only), ``joins`` (one base family) or ``bridges`` (two or
more base families become one); representative is the name of the combined family's smallest gene id; fused_base_families the
names of the base families' smallest genes, comma-separated (``-`` for none; a base gene that had no edge counts as a family of
one); collides is 1 when the combined family holds two genes of one genome that are not adjacent (the families tool would split
it), else 0.  ``--net`` writes the bytes ``python -m pandelos_amd.query -o`` writes for the same inputs.

This is NOT the clustering of a rebuilt union, in two ways: the base genomes' paralog thresholds can only fall once the new genome
exists, so a union run may add edges between base genes of one genome; and the union's last-record fold can change single
base-to-base cells.  ``python -m pandelos_amd.append`` commits.

``placement_from_edges`` is the contract in numpy: what ``pdl_place_query`` / ``pdl_placement_of_edges`` must return for a base
network and a query edge list.
"""
from __future__ import annotations

import argparse
import sys
from typing import Sequence

import numpy as np

from .pangene_idata import PangeneIData
from .pangenes import net_lines
from .query import QueryError, check_query

COUNTS = ("sequences", "n_query", "genomes", "groups", "novel", "joined", "bridging", "colliding", "unplaced")
ARRAYS = ("family_of", "is_node", "group_label", "group_query_off", "group_query", "group_base_off", "group_base", "group_collides")
STATUS = ("novel", "joins", "bridges")


def _components(n: int, src, dst):
    """Smallest member of every gene's component under the undirected edges (src, dst) over n genes."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(src, dst):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(n)], np.int64)


def placement_from_edges(base_src, base_dst, genome_of, n_query: int, src, dst) -> dict:
    """The placement of n_query query genes (union ids N.., one further genome) whose edges are (src, dst) on the base network
    (base_src, base_dst) over the N = len(genome_of) base genes -> the fields of ``pdl_placement`` (without the edges).

    Stated on the combined network itself: edges undirected, a repeated pair one edge, a self edge makes a node but no edge; a
    label is a component's smallest gene; a component collides when some genome has m >= 2 genes in it that are joined by fewer
    than m (m - 1) / 2 distinct edges."""
    genome_of = np.asarray(genome_of, np.int64)
    N, n = len(genome_of), int(n_query)
    G = int(genome_of.max()) + 1 if N else 0
    bs, bd = np.asarray(base_src, np.int64).tolist(), np.asarray(base_dst, np.int64).tolist()
    qs, qd = np.asarray(src, np.int64).tolist(), np.asarray(dst, np.int64).tolist()
    for a, b in zip(qs, qd):
        if not (0 <= a < N + n and 0 <= b < N + n) or (a < N and b < N):
            raise ValueError(f"query edge ({a}, {b}) names an id outside [0, {N + n}) or joins two base genes")
    genome = np.concatenate([genome_of, np.full(n, G, np.int64)])
    base_comp = _components(N, bs, bd)
    comp = _components(N + n, bs + qs, bd + qd)
    node = np.zeros(N + n, bool)
    node[bs + bd + qs + qd] = True
    pairs = {(min(a, b), max(a, b)) for a, b in zip(bs + qs, bd + qd) if a != b}
    is_node = node[N:]
    family_of = np.where(is_node, comp[N:], np.arange(N, N + n))
    labels = np.unique(family_of[is_node])
    # members per (component, genome) against the distinct edges inside that set
    held = {}
    for g in np.nonzero(node)[0].tolist():
        key = (int(comp[g]), int(genome[g]))
        held[key] = held.get(key, 0) + 1
    joined = {}
    for a, b in pairs:
        if genome[a] == genome[b]:
            key = (int(comp[a]), int(genome[a]))
            joined[key] = joined.get(key, 0) + 1
    colliding = {lab for (lab, _), m in held.items() if m >= 2 and joined.get((lab, _), 0) < m * (m - 1) // 2}
    q_members = {int(lab): [] for lab in labels}
    for i in np.nonzero(is_node)[0].tolist():
        q_members[int(family_of[i])].append(N + i)
    b_members = {int(lab): set() for lab in labels}         # the base components a group fuses (a base gene without an edge: its own)
    for g in range(N):
        if int(comp[g]) in b_members:
            b_members[int(comp[g])].add(int(base_comp[g]))
    group_query = [q_members[int(lab)] for lab in labels]
    group_base = [sorted(b_members[int(lab)]) for lab in labels]
    nb = np.array([len(x) for x in group_base], np.int64)
    collides = np.array([int(lab) in colliding for lab in labels], np.uint8)
    return {"sequences": N, "n_query": n, "genomes": G, "groups": len(labels), "novel": int((nb == 0).sum()), "joined": int((nb == 1).sum()),
            "bridging": int((nb >= 2).sum()), "colliding": int(collides.sum()), "unplaced": int(n - is_node.sum()),
            "family_of": family_of.astype(np.uint32), "is_node": is_node.astype(np.uint8), "group_label": labels.astype(np.uint32),
            "group_query_off": np.cumsum([0] + [len(x) for x in group_query]).astype(np.uint32),
            "group_query": np.array([g for x in group_query for g in x], np.uint32),
            "group_base_off": np.cumsum([0] + [len(x) for x in group_base]).astype(np.uint32),
            "group_base": np.array([g for x in group_base for g in x], np.uint32), "group_collides": collides}


def placement_rows(pl: dict, names: Sequence[str]):
    """One (gene, status, representative, fused base families, collides) row per query gene, names from ``names`` (union ids)."""
    N, n = int(pl["sequences"]), int(pl["n_query"])
    group_of = {int(lab): g for g, lab in enumerate(pl["group_label"].tolist())}
    b_off, base = pl["group_base_off"].tolist(), pl["group_base"].tolist()
    rows = []
    for i in range(n):
        if not pl["is_node"][i]:
            rows.append((names[N + i], "unplaced", names[N + i], "-", 0))
            continue
        g = group_of[int(pl["family_of"][i])]
        fused = base[b_off[g]:b_off[g + 1]]
        rows.append((names[N + i], STATUS[min(len(fused), 2)], names[int(pl["family_of"][i])],
                     ",".join(names[x] for x in fused) if fused else "-", int(pl["group_collides"][g])))
    return rows


def tsv_text(rows) -> str:
    return "".join(f"{a}\t{b}\t{c}\t{d}\t{e}\n" for a, b, c, d, e in rows)


def main(argv: Sequence[str] | None = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m pandelos_amd.place")
    ap.add_argument("-i", "--input", required=True, help="base set (.faa)")
    ap.add_argument("-k", "--kvalue", required=True, type=int, help="k-mer length (that of the base run)")
    ap.add_argument("-q", "--query", required=True, help="the new genome (.faa, one genome)")
    ap.add_argument("-o", "--output", required=True, help="one line per query gene: its family (.tsv)")
    ap.add_argument("--net", default=None, help="edges of the new genome's task (.net), as python -m pandelos_amd.query writes them")
    ap.add_argument("--rekey", action="store_true", help="accept letters the base lacks: rank the query in the union's alphabet (option query_rekey)")
    args = ap.parse_args(argv)

    base = PangeneIData.read_from_file(args.input)          # (names, and the label check)
    query = PangeneIData.read_from_file(args.query)
    try:
        check_query(query, base.genomeNames)
    except QueryError as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    from .pangene_native import PangeneNative
    nat = PangeneNative.open()
    try:
        ing = nat.ingest_faa(args.input)
        nat.preprocess_ingested(args.kvalue)
        if args.rekey:
            nat.set_option("query_rekey", 1)
        pl = nat.place_idata(query)
        info = nat.last_place_info
    finally:
        nat.close()
    with open(args.output, "w") as f:
        f.write(tsv_text(placement_rows(pl, list(base.sequenceName) + list(query.sequenceName))))
    if args.net:
        with open(args.net, "w") as f:
            f.writelines(net_lines(pl["src"], pl["dst"], pl["score"]))
    print(f"query genome '{query.genomeNames[0]}': {len(query.sequences)} genes against {ing['sequences']} base genes; {info['edges']} edges; "
          f"{pl['groups']} families touched: {pl['novel']} novel, {pl['joined']} joined, {pl['bridging']} bridging, {pl['colliding']} colliding; "
          f"{pl['unplaced']} genes unplaced -> {args.output}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
