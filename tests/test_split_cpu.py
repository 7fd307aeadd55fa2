"""The Girvan-Newman split off the device: the flat restatement of pdl_split_first_level's contract (tests/split_cases.py) against
netclu's loop, the level-by-level recursion against split_until_clean, the packing, and the reference fixtures."""
from __future__ import annotations

import numpy as np
import pytest

from pandelos_amd import netclu
from tests import helpers as H
from tests import split_cases as SC

NET, SPLIT = H.GOLDEN / "net", H.GOLDEN / "split"
PARALOGS = ("paralogs_6x80x120_k3", "paralogs_10x60x90_k3_div20")


def _names_of_clus(text):
    return sorted({n for line in text.splitlines() for n in line.split()})


def test_restatement_removes_what_netclu_removes():
    cases = {**SC.small_graphs(), **SC.chunk_edge_graphs()}
    for name, g in cases.items():
        got = SC.flat_on_graph(g)
        assert got == netclu.first_level_removals(g), name
        h = {u: dict(nb) for u, nb in g.items()}                      # ... and they are girvan_newman_first_level's own
        for u, v in got:
            del h[u][v]
            del h[v][u]
        assert netclu.connected_components(h) == netclu.girvan_newman_first_level(g), name
    for name, (g, want) in SC.beyond_lds_graphs().items():
        assert want == netclu.first_level_removals(g) and SC.lds_words(g) > SC.LDS_WORDS, name
    graphs, want = SC.random_expected()
    assert sum(len(w) for w in want) == 1549
    for seed, (g, w) in enumerate(zip(graphs, want)):
        assert w == netclu.first_level_removals(g), seed


def test_source_order_has_teeth():
    """Summing every edge's contributions in REVERSE source order changes the removed-edge sequence on 13 of the 400 random
    seeds (1 549 removals in all): the order the contract fixes is not cosmetic."""
    graphs, want = SC.random_expected()
    differ = [s for s, (g, w) in enumerate(zip(graphs, want)) if SC.flat_on_graph(g, reverse_sources=True) != w]
    print("seeds on which the reversed source order differs:", len(differ), differ)
    assert len(differ) >= 1


def test_pack_graphs_round_trip():
    graphs = list(SC.small_graphs().values()) + [SC.random_graph(s) for s in range(20)]
    node_off, adj_off, adj, keys = netclu.pack_graphs(graphs)
    assert node_off.dtype == np.uint64 and adj_off.dtype == np.uint64 and adj.dtype == np.uint32
    assert node_off[0] == 0 and adj_off[0] == 0 and len(adj_off) == node_off[-1] + 1 and adj_off[-1] == len(adj)
    back = netclu.unpack_graphs(node_off, adj_off, adj, keys)
    for g, h in zip(graphs, back):
        assert list(g) == list(h) and all(list(g[u]) == list(h[u]) for u in g)
    assert SC.flat_on_packing(node_off, adj_off, adj) == [[(k.index(u), k.index(v)) for u, v in SC.flat_on_graph(g)] for g, k in zip(graphs, keys)]
    empty = netclu.pack_graphs([])
    assert list(empty[0]) == [0] and list(empty[1]) == [0] and len(empty[2]) == 0 and empty[3] == []


def test_malformed_packings_are_built_once_and_differ_from_the_legal_one():
    (no, ao, ad), want = SC.legal_packing()
    # a triangle (three-way tie: the first edge, then the first of the path's two) and a path of 3 (tie: the first edge)
    assert want == [[(0, 1), (0, 2)], [(0, 1)]]
    assert want == [[(0, 1), (0, 2)], [(0, 1)]] == [netclu.first_level_removals(g) for g in netclu.unpack_graphs(no, ao, ad, [[0, 1, 2], [0, 1, 2]])]
    bad = SC.malformed_packings()
    assert len(bad) == 10
    for name, (n2, a2, d2) in bad.items():
        assert (n2, a2, d2) != (no.tolist(), ao.tolist(), ad.tolist()), name


def _colliding_filters(adj, genome_of):
    return [netclu.view_filter(c, adj.__contains__) for c in netclu.connected_components(adj) if netclu.max_collision(c, adj, genome_of) > 0]


@pytest.mark.parametrize("name,colliding", zip(PARALOGS, (51, 68)))
def test_level_by_level_is_the_recursion_on_the_paralog_fixtures(name, colliding, tmp_path):
    from pandelos_amd.synth import make_gene_set
    from tests.test_host_net import CASES
    faa = tmp_path / "in.faa"
    make_gene_set(**CASES[name][0]).write_faa(faa)
    names, genome_of = netclu.read_names(faa)
    adj = netclu.read_net(NET / f"{name}.net")
    filters = _colliding_filters(adj, genome_of)
    assert len(filters) == colliding
    calls = []

    def counted(graphs):
        calls.append(len(graphs))
        return netclu.host_first_level(graphs)
    got = netclu.split_all_until_clean(filters, adj, genome_of, None, counted)
    assert got == [netclu.split_until_clean(f, adj, genome_of) for f in filters]
    assert calls[0] == colliding and calls == sorted(calls, reverse=True)          # one call per level, all pending graphs in it
    # the .clus, byte for byte, with the level-by-level road in families()' place
    fams, placed = [], set()
    clean = [sorted(c) for c in netclu.connected_components(adj) if netclu.max_collision(c, adj, genome_of) == 0]
    for part in clean + [p for parts in got for p in parts]:
        fams.append(sorted(part))
        placed.update(part)
    singles = [g for g in range(len(names)) if g not in placed]
    assert netclu.clus_text(names, fams, singles) == (NET / f"{name}.clus").read_text()


def test_community_100_through_the_host_split():
    name = "community_100"
    names, genome_of = netclu.read_names(SPLIT / f"{name}.faa")
    adj = netclu.read_net(SPLIT / f"{name}.net")
    want = (SPLIT / f"{name}.clus").read_text()
    fams, singles = netclu.families(names, genome_of, adj)
    assert netclu.clus_text(names, fams, singles) == want
    filters = _colliding_filters(adj, genome_of)
    assert len(filters) == 1 and len(filters[0]) == 100
    assert netclu.split_all_until_clean(filters, adj, genome_of) == [netclu.split_until_clean(filters[0], adj, genome_of)]


def test_read_net_edges_gives_read_net_its_adjacency():
    path = SPLIT / "community_mixed.net"
    src, dst = netclu.read_net_edges(path)
    adj = {}
    for a, b in zip(src, dst):
        adj.setdefault(a, {})
        adj.setdefault(b, {})
        adj[a][b] = None
        adj[b][a] = None
    want = netclu.read_net(path)
    assert len(src) == len(path.read_text().splitlines()) and list(adj) == list(want) and all(list(adj[u]) == list(want[u]) for u in want)


def test_fixture_files_are_small_and_complete():
    for name, genes in (("community_100", 100), ("community_200", 200), ("community_mixed", 360)):
        for ext in ("faa", "net", "clus"):
            assert 0 < (SPLIT / f"{name}.{ext}").stat().st_size < 100_000
        assert len(_names_of_clus((SPLIT / f"{name}.clus").read_text())) == genes


def test_a_splitter_that_answers_short_or_leaves_a_graph_whole_is_refused():
    g = SC.small_graphs()["two triangles on a bridge"]
    genome_of = ["a", "b", "c", "a", "b", "c"]
    filt = netclu.view_filter(g, g.__contains__)
    assert netclu.max_collision(list(g), g, genome_of) > 0
    with pytest.raises(ValueError):
        netclu.split_all_until_clean([filt], g, genome_of, None, lambda graphs: [])
    with pytest.raises(ValueError):
        netclu.split_all_until_clean([filt], g, genome_of, None, lambda graphs: [[] for _ in graphs])
