"""The numpy statement of K-place's contract (pandelos_amd.place.placement_from_edges) against the script's own walk of the combined
network (netclu.connected_components / max_collision): every golden query fixture, base edges and query block from the CPU oracle and
the fixture, and hand-made graphs for each corner of the rules.  No GPU needed; tests/test_gpu_place.py holds the device to the same
statement and takes SHAPES and the helpers from here."""
import numpy as np
import pytest

from pandelos_amd import netclu
from pandelos_amd import place as P
from pandelos_amd.pangenes import bbh_edges
from pandelos_amd.scores import Scores
from tests import helpers as H
from tests.test_query_golden import CASES, load_case


def script_view(base_src, base_dst, genome_of, n, src, dst):
    """The placement as the script's walk of the combined network gives it: adjacency as read_net fills it, BFS components,
    max_collision; the base components from the base network alone."""
    N = len(genome_of)
    G = int(max(genome_of)) + 1 if N else 0
    genome = list(genome_of) + [G] * n

    def adjacency(pairs):
        adj = {}
        for a, b in pairs:
            adj.setdefault(a, {})
            if a != b:
                adj.setdefault(b, {})
                adj[a][b] = None
                adj[b][a] = None
        return adj
    base_pairs = list(zip(np.asarray(base_src).tolist(), np.asarray(base_dst).tolist()))
    adj = adjacency(base_pairs + list(zip(np.asarray(src).tolist(), np.asarray(dst).tolist())))
    base_label = {g: g for g in range(N)}
    for c in netclu.connected_components(adjacency(base_pairs)):
        for g in c:
            base_label[g] = min(c)
    family_of = np.arange(N, N + n, dtype=np.uint32)
    is_node = np.zeros(n, np.uint8)
    groups = []
    for c in sorted((sorted(c) for c in netclu.connected_components(adj)), key=lambda c: c[0]):
        q = [g for g in c if g >= N]
        if not q:
            continue
        family_of[np.array(q) - N] = c[0]
        is_node[np.array(q) - N] = 1
        groups.append((c[0], q, sorted({base_label[g] for g in c if g < N}), int(netclu.max_collision(c, adj, genome) > 0)))
    nb = np.array([len(g[2]) for g in groups], np.int64)
    return {"sequences": N, "n_query": n, "genomes": G, "groups": len(groups), "novel": int((nb == 0).sum()), "joined": int((nb == 1).sum()),
            "bridging": int((nb >= 2).sum()), "colliding": sum(g[3] for g in groups), "unplaced": int(n - is_node.sum()),
            "family_of": family_of, "is_node": is_node, "group_label": np.array([g[0] for g in groups], np.uint32),
            "group_query_off": np.cumsum([0] + [len(g[1]) for g in groups]).astype(np.uint32),
            "group_query": np.array([x for g in groups for x in g[1]], np.uint32),
            "group_base_off": np.cumsum([0] + [len(g[2]) for g in groups]).astype(np.uint32),
            "group_base": np.array([x for g in groups for x in g[2]], np.uint32), "group_collides": np.array([g[3] for g in groups], np.uint8)}


def assert_placement(got, want, label=""):
    for f in P.COUNTS:
        assert got[f] == want[f], f"{label}: {f} = {got[f]}, expected {want[f]}"
    for f in P.ARRAYS:
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), f"{label}: field {f} differs: {got[f]} != {want[f]}"


def _edges(pairs):
    return np.array([a for a, _ in pairs], np.int64), np.array([b for _, b in pairs], np.int64)


def shape(kind, wide=300):
    """-> (base_src, base_dst, genome_of, n_query, src, dst, expected statuses per group or None).  Base: families {0, 1} (genomes
    0, 1), {2, 3} (genomes 2, 3), {4, 5} (genomes 1, 2), {6, 7, 8} (genomes 0, 1, 0; 6 and 8 not adjacent: it collides); genes
    9, 10 (both genome 4) and 11 (genome 5) have no edge.  Query genes are N.."""
    base = [(0, 1), (2, 3), (4, 5), (6, 7), (7, 8)]
    genome_of = np.array([0, 1, 2, 3, 1, 2, 0, 1, 0, 4, 4, 5], np.uint32)
    N = 12
    q = {
        "no_query_edge": (3, [], []),
        "self_edge_only": (2, [(N + 1, N + 1)], [("novel", 0)]),
        "phase2_pair": (3, [(N, N + 2)], [("novel", 0)]),
        "two_join_adjacent": (2, [(0, N), (N + 1, 1), (N, N + 1)], [("joins", 0)]),
        "two_join_not_adjacent": (2, [(0, N), (N + 1, 1)], [("joins", 1)]),
        "bridge_disjoint_genomes": (1, [(N, 0), (N, 2)], [("bridges", 0)]),
        "bridge_shared_genome": (1, [(N, 0), (4, N)], [("bridges", 1)]),
        "bridge_onto_colliding": (2, [(N, 7), (N, 3), (N + 1, 6)], [("bridges", 1)]),
        "join_onto_colliding": (1, [(N, 7)], [("joins", 1)]),
        "join_non_node": (1, [(N, 11)], [("joins", 0)]),
        "bridge_two_non_nodes_one_genome": (1, [(N, 9), (10, N)], [("bridges", 1)]),
        "bridge_two_non_nodes_two_genomes": (1, [(N, 9), (11, N)], [("bridges", 0)]),
        "chain": (3, [(N, 0), (1, N + 1), (N + 1, 2), (3, N + 2), (N + 2, 11), (N, N + 1), (N + 1, N + 2), (N, N + 2)], [("bridges", 0)]),
        "chain_not_a_clique": (3, [(N, 0), (1, N + 1), (N + 1, 2), (3, N + 2), (N, N + 1), (N + 1, N + 2)], [("bridges", 1)]),
        "doubled_and_mirrored": (3, [(N, N + 1), (N + 1, N), (N, N + 1), (N, 0), (0, N), (N, 0), (N + 1, 1), (1, N + 1), (N + 2, N + 2), (N + 2, N + 2)],
                                 [("joins", 0), ("novel", 0)]),
    }
    if kind == "star":
        rng = np.random.default_rng(11)
        fams = wide
        base = [(2 * i, 2 * i + 1) for i in range(fams)] + [(2 * i + 1, 2 * i) for i in range(0, fams, 3)]
        genome_of = rng.integers(0, 64, 2 * fams + 5).astype(np.uint32)
        N = len(genome_of)
        hits = rng.permutation(fams)
        pairs = [(N + 1, 2 * int(i) + int(i) % 2) for i in hits] + [(2 * fams + 2, N + 1), (N, N + 2)]
        return (*_edges(base), genome_of, 4, *_edges(pairs), None)
    n, pairs, expect = q[kind]
    return (*_edges(base), genome_of, n, *_edges(pairs), expect)


SHAPES = ["no_query_edge", "self_edge_only", "phase2_pair", "two_join_adjacent", "two_join_not_adjacent", "bridge_disjoint_genomes",
          "bridge_shared_genome", "bridge_onto_colliding", "join_onto_colliding", "join_non_node", "bridge_two_non_nodes_one_genome",
          "bridge_two_non_nodes_two_genomes", "chain", "chain_not_a_clique", "doubled_and_mirrored", "star"]


def check_expectation(pl, expect, label):
    if expect is None:
        return
    nb = np.diff(pl["group_base_off"].astype(np.int64))
    got = [(P.STATUS[min(int(b), 2)], int(c)) for b, c in zip(nb, pl["group_collides"])]
    assert got == expect, f"{label}: {got} != {expect}"


@pytest.mark.parametrize("kind", SHAPES)
def test_hand_made_graphs(kind):
    bs, bd, genome_of, n, qs, qd, expect = shape(kind)
    got = P.placement_from_edges(bs, bd, genome_of, n, qs, qd)
    assert_placement(got, script_view(bs, bd, genome_of.tolist(), n, qs, qd), kind)
    check_expectation(got, expect, kind)
    if kind == "no_query_edge":
        assert got["groups"] == 0 and got["unplaced"] == 3 and got["family_of"].tolist() == [12, 13, 14]
    if kind == "self_edge_only":
        assert got["is_node"].tolist() == [0, 1] and got["group_label"].tolist() == [13] and got["unplaced"] == 1
    if kind == "join_non_node":
        assert got["group_base"].tolist() == [11] and got["family_of"].tolist() == [11]
    if kind == "chain":
        assert got["group_base"].tolist() == [0, 2, 11] and got["group_query"].tolist() == [12, 13, 14] and got["family_of"].tolist() == [0, 0, 0]
    if kind == "star":
        assert got["bridging"] == 1 and got["novel"] == 1 and len(got["group_base"]) == 301


def test_bad_edges_are_refused():
    bs, bd, genome_of, n, _, _, _ = shape("phase2_pair")
    for pair in [(0, 1)], [(12, 15)], [(-1, 12)]:
        with pytest.raises(ValueError):
            P.placement_from_edges(bs, bd, genome_of, n, *_edges(pair))


def oracle_case(name):
    """-> (base edges, genome_of of the base, n, the query's edges (src, dst, score)) of a golden query fixture: the base network from
    the CPU oracle on the base alone, the query's edges from the fixture's block."""
    from oracle import binding as ob
    fx, base, query, k, G = load_case(name)
    res_b, off_b, gen_b = base.flatten()
    ora = ob.Oracle(res_b, off_b, gen_b, k)
    parts = []
    for g in range(G):
        s = ora.scores(g)
        parts.append(bbh_edges(Scores(scoresCount=int(s["scoresCount"]), **{f: np.asarray(s[f]) for f in H.FIELDS})))
    bs, bd = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    floats = ("scores", "percs", "tr_percs", "max_genome_score", "max_genome_score_col")        # (stored as their bit patterns)
    block = Scores(scoresCount=len(fx["scores"]), **{f: fx[f].view(np.float32) if f in floats else fx[f] for f in H.FIELDS})
    return (bs, bd), gen_b, len(query.sequences), bbh_edges(block)


@pytest.mark.parametrize("name", CASES)
def test_fixtures_against_the_script(name):
    (bs, bd), gen_b, n, (qs, qd, _) = oracle_case(name)
    got = P.placement_from_edges(bs, bd, gen_b, n, qs, qd)
    assert_placement(got, script_view(bs, bd, gen_b.tolist(), n, qs, qd), name)
    assert got["novel"] + got["joined"] + got["bridging"] == got["groups"] and got["unplaced"] == n - int(got["is_node"].sum())


def test_rows_and_text():
    bs, bd, genome_of, n, qs, qd, _ = shape("doubled_and_mirrored")
    names = [f"b{i}" for i in range(12)] + ["q0", "q1", "q2"]
    rows = P.placement_rows(P.placement_from_edges(bs, bd, genome_of, n, qs, qd), names)
    assert rows == [("q0", "joins", "b0", "b0", 0), ("q1", "joins", "b0", "b0", 0), ("q2", "novel", "q2", "-", 0)]
    bs, bd, genome_of, n, qs, qd, _ = shape("bridge_onto_colliding")
    rows = P.placement_rows(P.placement_from_edges(bs, bd, genome_of, n, qs, qd), names)
    assert P.tsv_text(rows) == "q0\tbridges\tb2\tb2,b6\t1\nq1\tbridges\tb2\tb2,b6\t1\n"
    bs, bd, genome_of, n, qs, qd, _ = shape("no_query_edge")
    assert P.placement_rows(P.placement_from_edges(bs, bd, genome_of, n, qs, qd), names)[0] == ("q0", "unplaced", "q0", "-", 0)
