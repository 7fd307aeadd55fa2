"""K-fam's contract and its host half, without a device.

``families_contract`` is a numpy statement of what ``pdl_families`` (include/pandelos_amd.h) holds for an edge list: a
component's label is its smallest gene id, a gene is a node when any edge names it (a self edge too), families come in
ascending order of their labels with ascending members, and a component collides by the rule of netclu_ng.py:75-92 — two
of its genes belong to one genome and are not adjacent.  Fed through ``netclu.families_from_components`` together with the
fixture networks it must give the ``.clus`` fixtures (the reference's own netclu_ng.py made them) byte for byte; so the host
half that splits only the colliding components is pinned to the reference, and the GPU tests (tests/test_gpu_families.py)
only have to show that the device fills the struct this way."""
import gzip
import json

import numpy as np
import pytest

from pandelos_amd import netclu
from pandelos_amd import pangenes as PH
from pandelos_amd.synth import make_gene_set
from tests import helpers as H
from tests.test_host_net import CASES, _OracleNative

NET = H.GOLDEN / "net"


def families_contract(src, dst, genome_of, n):
    """-> the dict ``PangeneNative.generate_families`` returns, from numpy alone."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    genome_of = np.asarray(genome_of)
    is_node = np.zeros(n, np.uint8)
    is_node[src] = 1
    is_node[dst] = 1
    lo, hi = np.minimum(src, dst), np.maximum(src, dst)
    pair = np.unique((lo << 32 | hi)[lo != hi])                     # undirected, one edge per pair, no self edge
    lo, hi = pair >> 32, pair & 0xFFFFFFFF
    label = np.arange(n, dtype=np.int64)
    while True:                                                     # smallest id of the component: relax over the edges, then jump
        new = label.copy()
        m = np.minimum(label[lo], label[hi])
        np.minimum.at(new, lo, m)
        np.minimum.at(new, hi, m)
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    nodes = np.nonzero(is_node)[0]
    order = nodes[np.argsort(label[nodes], kind="stable")]          # (label, gene)
    labels, start = np.unique(label[order], return_index=True)
    family_off = np.append(start, len(order)).astype(np.uint32)
    # collision: in a component, m >= 2 genes of one genome of which one has fewer than m - 1 neighbours of that genome
    same = genome_of[lo] == genome_of[hi]
    same_deg = np.bincount(np.concatenate([lo[same], hi[same]]), minlength=n)
    group = label[nodes] * (int(genome_of.max()) + 1 if n else 1) + genome_of[nodes]
    _, inv, cnt = np.unique(group, return_inverse=True, return_counts=True)
    bad_gene = same_deg[nodes] != cnt[inv] - 1
    collides = np.isin(labels, label[nodes][bad_gene]).astype(np.uint8)
    return {"sequences": n, "nodes": len(nodes), "families": len(labels), "colliding": int(collides.sum()),
            "component_of": label.astype(np.uint32), "is_node": is_node, "family_off": family_off,
            "family_genes": order.astype(np.uint32), "collides": collides}


def _net_edges(text):
    cols = np.array([l.split("\t")[:2] for l in text.splitlines() if l.strip()], dtype=np.int64).reshape(-1, 2)
    return cols[:, 0], cols[:, 1]


def _names_and_genomes(shape, tmp_path):
    gs = make_gene_set(**shape)
    faa = tmp_path / "in.faa"
    gs.write_faa(faa)
    names, genome_names = netclu.read_names(faa)
    return gs, names, genome_names


@pytest.mark.parametrize("name", sorted(CASES))
def test_contract_and_host_half_give_the_reference_clus_from_the_net(name, tmp_path):
    shape, _ = CASES[name]
    gs, names, genome_names = _names_and_genomes(shape, tmp_path)
    src, dst = _net_edges((NET / f"{name}.net").read_text())
    fam = families_contract(src, dst, gs.genome_of, gs.genes)
    fams, singles = netclu.families_from_components(names, genome_names, fam, src, dst, net_ordered=True)
    assert netclu.clus_text(names, fams, singles) == (NET / f"{name}.clus").read_text()
    if name.startswith("paralogs"):
        assert 0 < fam["colliding"] < fam["families"]              # both roads are taken


@pytest.mark.parametrize("name", sorted(CASES))
def test_contract_and_host_half_give_the_reference_clus_from_the_edges(name, tmp_path):
    """The same from the edges in insertion order (what the device hands over), the line order derived by the function
    that also orders the ``.net`` text — which still is the fixture's."""
    shape, k = CASES[name]
    gs, names, genome_names = _names_and_genomes(shape, tmp_path)
    nat = _OracleNative(gs, k)
    parts = [PH.bbh_edges(nat.generate_scores_part(g)) for g in range(gs.genomes)]
    src, dst, sc = (np.concatenate([p[i] for p in parts]) for i in range(3))
    assert "".join(PH.net_lines(src, dst, sc)) == (NET / f"{name}.net").read_text()
    order = PH.net_line_order(src, dst)
    assert [f"{a}\t{b}" for a, b in zip(src[order], dst[order])] == [l.rsplit("\t", 1)[0] for l in (NET / f"{name}.net").read_text().splitlines()]
    fam = families_contract(src, dst, gs.genome_of, gs.genes)
    fams, singles = netclu.families_from_components(names, genome_names, fam, src, dst)
    assert netclu.clus_text(names, fams, singles) == (NET / f"{name}.clus").read_text()


@pytest.mark.timeout(600)
def test_canonical_64_genome_set(tmp_path):
    name = "mycoplasma64_standin"
    shape = json.loads((H.GOLDEN / "digests_baseline.json").read_text())[name]["shape"]
    gs, names, genome_names = _names_and_genomes(shape, tmp_path)
    src, dst = _net_edges(gzip.open(NET / f"{name}.net.gz", "rt").read())
    fam = families_contract(src, dst, gs.genome_of, gs.genes)
    assert (fam["nodes"], fam["families"], fam["colliding"]) == (38590, 931, 0)
    fams, singles = netclu.families_from_components(names, genome_names, fam, src, dst, net_ordered=True)
    assert netclu.clus_text(names, fams, singles) == gzip.open(NET / f"{name}.clus.gz", "rt").read()


def test_contract_against_the_scripts_components_and_collisions(tmp_path):
    """The numpy statement itself against netclu.connected_components / max_collision (the restatement of the script)."""
    for name in ("paralogs_6x80x120_k3", "synth_5x60x80_k3"):
        shape, _ = CASES[name]
        gs = make_gene_set(**shape)
        src, dst = _net_edges((NET / f"{name}.net").read_text())
        fam = families_contract(src, dst, gs.genome_of, gs.genes)
        adj = netclu.read_net(NET / f"{name}.net")
        comps = sorted(netclu.connected_components(adj), key=min)
        assert fam["nodes"] == len(adj) and fam["families"] == len(comps)
        for f, comp in enumerate(comps):
            assert fam["family_genes"][fam["family_off"][f]:fam["family_off"][f + 1]].tolist() == sorted(comp)
            assert all(fam["component_of"][g] == min(comp) for g in comp)
            assert bool(fam["collides"][f]) == (netclu.max_collision(sorted(comp), adj, gs.genome_of) > 0)


def test_two_triangles_and_a_bridge_and_odd_edges():
    genome_of = np.array([0, 1, 2, 0, 1, 2, 0, 0], np.uint32)
    e = [(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5), (2, 3), (3, 2), (2, 3), (6, 6)]      # a pair three times, a self edge
    src, dst = np.array([a for a, _ in e]), np.array([b for _, b in e])
    fam = families_contract(src, dst, genome_of, 8)
    assert fam["nodes"] == 7 and fam["families"] == 2 and fam["collides"].tolist() == [1, 0]
    assert fam["family_off"].tolist() == [0, 6, 7] and fam["family_genes"].tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert fam["component_of"].tolist() == [0, 0, 0, 0, 0, 0, 6, 7] and fam["is_node"].tolist() == [1] * 7 + [0]
    names = [f"g{i}" for i in range(8)]
    fams, singles = netclu.families_from_components(names, genome_of.tolist(), fam, src, dst)
    assert sorted(fams) == [[0, 1, 2], [3, 4, 5], [6]] and singles == [7]
    assert netclu.clus_text(names, fams, singles) == "g0 g1 g2\ng3 g4 g5\ng6\ng7 \n"
