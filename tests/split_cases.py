"""Cases of the Girvan-Newman split (pdl_split_first_level, pandelos_amd/csrc/pdl_split.h) and a flat restatement of its contract.

``flat_first_level`` states the contract of include/pandelos_amd.h on the PACKED arrays alone: local indices, one removed mark per
slot, plain Python floats (IEEE doubles, every product rounded before it is added), every edge's sum taken in source order.  It
knows nothing of netclu's dicts; tests/test_split_cpu.py holds it against ``netclu.first_level_removals`` on every case below,
tests/test_gpu_split.py holds the device against it.
"""
from __future__ import annotations

import random
from functools import lru_cache
from typing import Dict, List, Tuple

import numpy as np

from pandelos_amd import netclu

Adj = Dict[int, Dict[int, None]]


# ---- generators ----------------------------------------------------------------------------------------------------------------
def graph_of(nodes, edges) -> Adj:
    """Nodes in the order given, every edge entered in both directions in the order given (as netclu.read_net fills a network),
    then rebuilt twice as girvan_newman_first_level does."""
    g: Adj = {u: {} for u in nodes}
    for a, b in edges:
        g[a][b] = None
        g[b][a] = None
    return netclu.rebuilt(netclu.rebuilt(g))


def path(n): return graph_of(range(n), [(i, i + 1) for i in range(n - 1)])
def cycle(n): return graph_of(range(n), [(i, (i + 1) % n) for i in range(n)])
def star(n): return graph_of(range(n), [(0, i) for i in range(1, n)])
def complete(n): return graph_of(range(n), [(i, j) for i in range(n) for j in range(i + 1, n)])
def hypercube(d): return graph_of(range(1 << d), [(i, i ^ (1 << b)) for i in range(1 << d) for b in range(d) if i < i ^ (1 << b)])


def small_graphs() -> Dict[str, Adj]:
    return {
        "one edge": path(2),
        "path of 3": path(3),
        "triangle": cycle(3),
        "4-cycle": cycle(4),
        "star": star(6),
        "K4": complete(4),
        "two triangles on a bridge": graph_of(range(6), [(0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 3), (2, 3)]),
        "K3,3": graph_of(range(6), [(i, j) for i in range(3) for j in range(3, 6)]),
        "Q3": hypercube(3),
        "Q4": hypercube(4),
        "one node": graph_of([7], []),
    }


CHUNK_SIZES = (63, 64, 65, 255, 256, 257)


def chunk_edge_graphs() -> Dict[str, Adj]:
    out = {}
    for n in CHUNK_SIZES:
        out[f"path of {n}"] = path(n)
        out[f"cycle of {n}"] = cycle(n)
    return out


def two_cliques(k: int, paths) -> Adj:
    """Two K_k (nodes 0 .. k-1 and k .. 2k-1) joined by one path per entry of ``paths``: entry j is the number of nodes in
    between (0: a bridge edge); path p starts at node p of the first clique and ends at node k + p of the second."""
    edges = [(a + i, a + j) for a in (0, k) for i in range(k) for j in range(i + 1, k)]
    nxt = 2 * k
    for p, between in enumerate(paths):
        chain = [p] + list(range(nxt, nxt + between)) + [k + p]
        nxt += between
        edges += list(zip(chain, chain[1:]))
    return graph_of(range(nxt), edges)


LDS_WORDS = 12288          # SPLIT_LDS_WORDS of pdl_split.h: the adjacency sits in LDS while n + 1 + 4 m <= this


def lds_words(g: Adj) -> int:
    return len(g) + 1 + 4 * len(netclu.edge_list(g))


@lru_cache(maxsize=None)
def beyond_lds_graphs():
    """Graphs whose adjacency does NOT fit the kernel's LDS (the removed marks then live in the workgroup's scratch, offsets and
    edge ids are read from global memory), each with what the restatement removes: two K56 on a bridge (one removal), and on
    two and on three parallel paths (the marks are walked by the rounds that follow the first)."""
    out = {"two K56 on a bridge": two_cliques(56, [0]), "two K56 on two paths": two_cliques(56, [1, 1]),
           "two K56 on three paths": two_cliques(56, [0, 1, 2])}
    return {name: (g, flat_on_graph(g)) for name, g in out.items()}


def random_graph(seed: int) -> Adj:
    """The issue's random case: n = randrange(6, 28), ids 100 .. 100 + n - 1 shuffled, a ring in that order, randrange(0, 2 n)
    random pairs on top (self pairs ignored)."""
    rng = random.Random(seed)
    n = rng.randrange(6, 28)
    ids = list(range(100, 100 + n))
    rng.shuffle(ids)
    edges = [(ids[i], ids[(i + 1) % n]) for i in range(n)]
    for _ in range(rng.randrange(0, 2 * n)):
        a, b = rng.choice(ids), rng.choice(ids)
        if a != b:
            edges.append((a, b))
    return graph_of(ids, edges)


RANDOM_SEEDS = range(400)


def two_community_edges(n: int, seed: int, degree: int = 9, cross: float = 0.03) -> List[Tuple[int, int]]:
    """One component of n nodes: a ring through all of them plus random pairs, `cross` of them across the two halves, average
    degree about `degree` (the graphs the issue timed)."""
    rng = random.Random(seed)
    edges = [(i, (i + 1) % n) for i in range(n)]
    have = {(min(a, b), max(a, b)) for a, b in edges}
    half = n // 2
    while len(have) < n * degree // 2:
        if rng.random() < cross:
            a, b = rng.randrange(0, half), rng.randrange(half, n)
        else:
            lo = 0 if rng.random() < 0.5 else half
            a, b = rng.randrange(lo, lo + half), rng.randrange(lo, lo + half)
        if a != b and (min(a, b), max(a, b)) not in have:
            have.add((min(a, b), max(a, b)))
            edges.append((a, b))
    return edges


# ---- the contract on the packed arrays -----------------------------------------------------------------------------------------
def flat_first_level(n: int, adj_off, adj, reverse_sources: bool = False) -> List[Tuple[int, int]]:
    """One graph of a packing (adj_off from 0, local indices) -> removed edges (u < v) in removal order."""
    adj_off, adj = [int(x) for x in adj_off], [int(x) for x in adj]
    gone = [False] * len(adj)
    slot_edge, ends, slots = [0] * len(adj), [], {}
    for u in range(n):                                      # the edge list: slots that point to a later node, in slot order
        for k in range(adj_off[u], adj_off[u + 1]):
            if adj[k] > u:
                slots[(u, adj[k])] = len(ends)
                slot_edge[k] = len(ends)
                ends.append((u, adj[k], k))
    back = {}
    for u in range(n):
        for k in range(adj_off[u], adj_off[u + 1]):
            if adj[k] < u:
                slot_edge[k] = slots[(adj[k], u)]
                back[slot_edge[k]] = k
    m, removed = len(ends), []
    if m == 0:
        return removed
    alive = [True] * m
    scale = 1 / (n * (n - 1))
    for _ in range(m):
        per_source = []
        for s in range(n):
            dist, sigma, delta, order = [-1] * n, [0.0] * n, [0.0] * n, [s]
            dist[s], sigma[s] = 0, 1.0
            head = 0
            while head < len(order):
                v = order[head]; head += 1
                for k in range(adj_off[v], adj_off[v + 1]):
                    if gone[k]:
                        continue
                    w = adj[k]
                    if dist[w] < 0:
                        order.append(w)
                        dist[w] = dist[v] + 1
                    if dist[w] == dist[v] + 1:
                        sigma[w] += sigma[v]
            c_of = {}
            for w in reversed(order):
                coeff = (1 + delta[w]) / sigma[w]
                for k in range(adj_off[w], adj_off[w + 1]):
                    v = adj[k]
                    if gone[k] or dist[v] + 1 != dist[w]:
                        continue
                    c = sigma[v] * coeff
                    c_of[slot_edge[k]] = c
                    delta[v] += c
            per_source.append(c_of)
        bet = [0.0] * m
        for c_of in (reversed(per_source) if reverse_sources else per_source):
            for e, c in c_of.items():
                bet[e] += c
        best = None
        for e in range(m):
            if alive[e] and (best is None or bet[e] * scale > bet[best] * scale):
                best = e
        u, v, k = ends[best]
        alive[best] = False
        gone[k] = gone[back[best]] = True
        removed.append((u, v))
        seen, stack = {u}, [u]
        while stack:
            x = stack.pop()
            for k in range(adj_off[x], adj_off[x + 1]):
                if not gone[k] and adj[k] not in seen:
                    seen.add(adj[k]); stack.append(adj[k])
        if v not in seen:
            return removed
    return removed


def flat_on_graph(g: Adj, reverse_sources: bool = False) -> List[Tuple[int, int]]:
    """``flat_first_level`` of one ordered adjacency, the edges named by its nodes."""
    node_off, adj_off, adj, keys = netclu.pack_graphs([g])
    return [(keys[0][u], keys[0][v]) for u, v in flat_first_level(len(g), adj_off, adj, reverse_sources)]


def flat_on_packing(node_off, adj_off, adj) -> List[List[Tuple[int, int]]]:
    """Every graph of a packing -> removed edges in local indices (what PangeneNative.split_packed returns)."""
    out = []
    for j in range(len(node_off) - 1):
        a, b = int(node_off[j]), int(node_off[j + 1])
        s0 = int(adj_off[a])
        out.append(flat_first_level(b - a, [int(x) - s0 for x in adj_off[a:b + 1]], adj[s0:int(adj_off[b])]))
    return out


@lru_cache(maxsize=None)
def random_expected():
    """The 400 random graphs and what the restatement removes from each (computed once, shared, not to be changed)."""
    graphs = [random_graph(s) for s in RANDOM_SEEDS]
    return graphs, [flat_on_graph(g) for g in graphs]


# ---- malformed packings (every refusal of the contract; built once, sent by the GPU test) ---------------------------------------
def malformed_packings() -> Dict[str, tuple]:
    """name -> (node_off, adj_off, adj) as Python lists; each is a triangle + a path of 3 with one thing wrong."""
    node_off, adj_off, adj = [0, 3, 6], [0, 2, 4, 6, 7, 9, 10], [1, 2, 0, 2, 1, 0, 1, 0, 2, 1]

    def with_(no=None, ao=None, ad=None):
        return (list(no or node_off), list(ao or adj_off), list(ad or adj))
    return {
        "node_off does not start at 0": with_(no=[1, 3, 6]),
        "node_off decreases": with_(no=[0, 4, 3]),
        "adj_off does not start at 0": with_(ao=[1, 2, 4, 6, 7, 9, 10]),
        "adj_off decreases": with_(ao=[0, 2, 1, 6, 7, 9, 10]),
        "neighbour outside its graph": with_(ad=[1, 2, 0, 2, 1, 0, 1, 0, 3, 1]),
        "neighbour index huge": with_(ad=[1, 2, 0, 2, 1, 0, 1, 0, 0xffffffff, 1]),
        "self loop": with_(ad=[1, 2, 0, 2, 1, 0, 1, 0, 1, 1]),
        "neighbour named twice": with_(ad=[1, 1, 0, 2, 1, 0, 1, 0, 2, 1]),
        "edge in one direction only": with_(ao=[0, 2, 4, 6, 7, 9, 9], ad=[1, 2, 0, 2, 1, 0, 1, 0, 2]),
        "edge in one direction only, counts equal": with_(ad=[1, 2, 0, 2, 1, 0, 2, 0, 2, 1]),
    }


def legal_packing():
    """The packing the malformed ones are made from, and its answer."""
    node_off, adj_off, adj = [0, 3, 6], [0, 2, 4, 6, 7, 9, 10], [1, 2, 0, 2, 1, 0, 1, 0, 2, 1]
    arrays = (np.asarray(node_off, np.uint64), np.asarray(adj_off, np.uint64), np.asarray(adj, np.uint32))
    return arrays, flat_on_packing(*arrays)
