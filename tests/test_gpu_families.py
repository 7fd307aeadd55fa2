"""K-fam on the device (pdl_compute_families / pdl_families_of_edges, pandelos_amd/csrc/pdl_families.h).

  * reference-pinned: ``python -m pandelos_amd.families`` writes the ``.clus`` fixtures the reference's own netclu_ng.py made;
  * field by field: every field of ``pdl_families`` against netclu.connected_components / max_collision (the restatement of
    the script) on the context's own pdl_compute_edges edges, fixture sets and random ones;
  * graph shapes no tiny gene set produces, through pdl_families_of_edges, against a host union-find written here;
  * state: idempotent, nothing else of the context moves, append = union, refusals return their code."""
import gzip
import json
import os

import numpy as np
import pytest

from pandelos_amd import _lib, netclu
from pandelos_amd import families as FAM
from pandelos_amd.synth import make_gene_set
from tests import helpers as H
from tests.test_host_net import CASES

pytestmark = pytest.mark.gpu
NET = H.GOLDEN / "net"
CANON = "mycoplasma64_standin"
SEEDS = int(os.environ.get("PDL_FAMILIES_SEEDS", "60"))
ARRAYS = ("component_of", "is_node", "family_off", "family_genes", "collides")
COUNTS = ("sequences", "nodes", "families", "colliding")


def _shape_and_k(name):
    if name == CANON:
        d = json.loads((H.GOLDEN / "digests_baseline.json").read_text())[name]
        return d["shape"], d["k"]
    return CASES[name]


def _fixture_clus(name):
    return gzip.open(NET / f"{name}.clus.gz", "rt").read() if name == CANON else (NET / f"{name}.clus").read_text()


def random_shape(seed):
    """Small sets, every second one with paralogs.  On the CPU oracle the 60 default seeds hold 691 colliding and 2585 clean
    components and 1934 genes that are no node (low presence leaves genes without a partner)."""
    rng = np.random.default_rng(9000 + seed)
    return dict(genomes=int(rng.integers(3, 8)), genes_per_genome=int(rng.integers(20, 61)), mean_len=int(rng.integers(50, 111)),
                sub_rate=float(rng.uniform(0.05, 0.3)), presence=float(rng.uniform(0.6, 0.9)), seed=7000 + seed,
                paralogs=0.4 if seed % 2 else 0.0), 3


def _native(gs, k):
    from pandelos_amd.pangene_native import PangeneNative
    return PangeneNative.from_arrays(k, gs.residues, gs.offsets, gs.genome_of)


def _script_view(src, dst, genome_of, n):
    """The struct as the script's own walk gives it: adjacency as read_net fills it, BFS components, max_collision."""
    adj = {}
    for a, b in zip(src.tolist(), dst.tolist()):
        adj.setdefault(a, {})
        if a != b:
            adj.setdefault(b, {})
            adj[a][b] = None
            adj[b][a] = None
    comps = sorted((sorted(c) for c in netclu.connected_components(adj)), key=lambda c: c[0])
    component_of = np.arange(n, dtype=np.uint32)
    is_node = np.zeros(n, np.uint8)
    for c in comps:
        component_of[c] = c[0]
        is_node[c] = 1
    collides = np.array([netclu.max_collision(c, adj, genome_of) > 0 for c in comps], np.uint8)
    return {"sequences": n, "nodes": len(adj), "families": len(comps), "colliding": int(collides.sum()), "component_of": component_of,
            "is_node": is_node, "family_off": np.cumsum([0] + [len(c) for c in comps]).astype(np.uint32),
            "family_genes": np.array([g for c in comps for g in c], np.uint32), "collides": collides}


def _assert_same(got, want, label=""):
    for f in COUNTS:
        assert got[f] == want[f], f"{label}: {f} = {got[f]}, expected {want[f]}"
    for f in ARRAYS:
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), f"{label}: field {f} differs"


def _check_against_script(nat, gs, label):
    src, dst, _ = FAM.gather_edges(nat, gs.genomes)
    got = nat.generate_families()
    want = _script_view(src, dst, gs.genome_of.tolist(), gs.genes)
    _assert_same(got, want, label)
    return want


# ---- reference-pinned ------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
@pytest.mark.parametrize("name", sorted(CASES) + [CANON])
def test_command_writes_the_reference_clus(name, tmp_path):
    shape, k = _shape_and_k(name)
    faa, clus = tmp_path / "in.faa", tmp_path / "out.clus"
    make_gene_set(**shape).write_faa(faa)
    assert FAM.main(["-i", str(faa), "-k", str(k), "-o", str(clus)]) == 0
    assert clus.read_text() == _fixture_clus(name)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.faa", "out.clus"]          # no .net on the way


def test_command_with_auto_k_and_a_net(tmp_path):
    name = "paralogs_6x80x120_k3"
    shape, k = CASES[name]
    faa, clus, net = tmp_path / "in.faa", tmp_path / "out.clus", tmp_path / "out.net"
    make_gene_set(**shape).write_faa(faa)
    assert FAM.main(["-i", str(faa), "-k", "auto", "-o", str(clus), "--net", str(net)]) == 0
    from pandelos_amd.calculate_k import calculate_k_faa
    assert calculate_k_faa(faa) == k
    assert clus.read_text() == _fixture_clus(name) and net.read_text() == (NET / f"{name}.net").read_text()


# ---- field by field --------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
@pytest.mark.parametrize("name", sorted(CASES) + [CANON])
def test_fields_on_the_fixture_sets(name):
    shape, k = _shape_and_k(name)
    gs = make_gene_set(**shape)
    want = _check_against_script(_native(gs, k), gs, name)
    if name == CANON:
        assert (want["nodes"], want["families"], want["colliding"]) == (38590, 931, 0)


@pytest.mark.timeout(1800)
def test_fields_on_random_sets():
    seen = np.zeros(3, np.int64)                      # colliding components, clean ones, genes that are no node
    for seed in range(SEEDS):
        shape, k = random_shape(seed)
        gs = make_gene_set(**shape)
        want = _check_against_script(_native(gs, k), gs, f"seed {seed} {shape}")
        seen += [want["colliding"], want["families"] - want["colliding"], gs.genes - want["nodes"]]
    assert (seen > 0).all(), seen


# ---- graph shapes through pdl_families_of_edges ----------------------------------------------------------------------------
def _host_union_find(src, dst, genome_of, n):
    """Union-find with path halving on the host, hooking the larger root under the smaller; collisions by counting, per gene, its
    distinct neighbours of its own genome against the size of its (component, genome) group."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    is_node = np.zeros(n, np.uint8)
    pairs = set()
    for a, b in zip(src.tolist(), dst.tolist()):
        is_node[a] = is_node[b] = 1
        if a == b:
            continue
        pairs.add((min(a, b), max(a, b)))
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    component_of = np.array([find(i) for i in range(n)], np.uint32)
    nodes = np.nonzero(is_node)[0]
    order = nodes[np.argsort(component_of[nodes], kind="stable")]
    labels, start = np.unique(component_of[order], return_index=True)
    same_deg = np.zeros(n, np.int64)
    for a, b in pairs:
        if genome_of[a] == genome_of[b]:
            same_deg[a] += 1
            same_deg[b] += 1
    group = {}
    for g in nodes.tolist():
        group.setdefault((component_of[g], genome_of[g]), []).append(g)
    bad = {lab for (lab, _), members in group.items() if any(same_deg[g] != len(members) - 1 for g in members)}
    collides = np.array([lab in bad for lab in labels.tolist()], np.uint8)
    return {"sequences": n, "nodes": len(nodes), "families": len(labels), "colliding": int(collides.sum()), "component_of": component_of,
            "is_node": is_node, "family_off": np.append(start, len(order)).astype(np.uint32), "family_genes": order.astype(np.uint32),
            "collides": collides}


@pytest.fixture(scope="module")
def ctx():
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.open()                        # no preprocess: pdl_families_of_edges needs none
    yield nat
    nat.close()


def _graph(kind):
    rng = np.random.default_rng(5)
    n = 1 << 20
    if kind in ("path_shuffled", "path_descending"):
        a = np.arange(n - 1)
        src, dst = a, a + 1
        perm = rng.permutation(n - 1) if kind == "path_shuffled" else a[::-1]
        flip = rng.random(n - 1) < 0.5 if kind == "path_shuffled" else np.ones(n - 1, bool)
        src, dst = np.where(flip, dst, src)[perm], np.where(flip, src, dst)[perm]
        return src, dst, (np.arange(n) % 5).astype(np.uint32), n
    if kind == "star":
        leaves = rng.permutation(np.arange(1, n + 1))
        return np.where(leaves % 2 == 0, 0, leaves), np.where(leaves % 2 == 0, leaves, 0), (np.arange(n + 1) % 3).astype(np.uint32), n + 1
    if kind == "triangles":
        t = 100000
        b = 3 * rng.permutation(t)
        src, dst = np.concatenate([b, b + 1, b + 2]), np.concatenate([b + 1, b + 2, b])
        genome_of = np.tile(np.array([0, 1, 2], np.uint32), t)
        genome_of[3 * np.arange(0, t, 7) + 1] = 0           # every seventh triangle holds two adjacent genes of genome 0: still clean
        return src, dst, genome_of, 3 * t
    if kind == "twice_and_both_ways":
        m, n = 30000, 20000
        a, b = rng.integers(0, n, m), rng.integers(0, n, m)
        return np.concatenate([a, b, a, b]), np.concatenate([b, a, b, a]), rng.integers(0, 4, n).astype(np.uint32), n
    if kind == "self_edges":
        src, dst = np.array([0, 1, 3, 3, 5, 6, 6]), np.array([1, 1, 3, 3, 6, 5, 6])      # 3: only self edges; 1, 6: a self edge beside a real one
        return src, dst, np.array([0, 0, 1, 0, 1, 2, 2, 0], np.uint32), 8
    if kind == "bridge":
        e = [(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5), (2, 3)]
        return np.array([a for a, _ in e]), np.array([b for _, b in e]), np.array([0, 1, 2, 0, 1, 2], np.uint32), 6
    if kind in ("clique", "clique_minus_one"):
        m = 40
        a, b = np.triu_indices(m, 1)
        keep = np.ones(len(a), bool)
        if kind == "clique_minus_one":
            keep[(a == 7) & (b == 23)] = False
        p = rng.permutation(int(keep.sum()))
        return a[keep][p] + 2, b[keep][p] + 2, np.full(m + 4, 1, np.uint32), m + 4
    raise KeyError(kind)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("kind", ["path_shuffled", "path_descending", "star", "triangles", "twice_and_both_ways", "self_edges", "bridge", "clique",
                                  "clique_minus_one"])
def test_graph_shapes(kind, ctx):
    src, dst, genome_of, n = _graph(kind)
    got = ctx.families_of_edges(src, dst, genome_of)
    want = _host_union_find(np.asarray(src), np.asarray(dst), genome_of.tolist(), n)
    _assert_same(got, want, kind)
    if kind in ("path_shuffled", "path_descending", "star"):
        assert got["families"] == 1 and got["nodes"] == n and not got["component_of"].any() and got["colliding"] == 1
    if kind == "triangles":
        assert got["families"] == 100000 and got["colliding"] == 0
    if kind == "self_edges":
        assert got["family_off"].tolist() == [0, 2, 3, 5] and got["family_genes"].tolist() == [0, 1, 3, 5, 6] and got["colliding"] == 0
    if kind == "bridge":
        assert got["collides"].tolist() == [1]
        names = [f"g{i}" for i in range(6)]
        fams, singles = netclu.families_from_components(names, ["A", "B", "C", "A", "B", "C"], got, src, dst)
        assert sorted(fams) == [[0, 1, 2], [3, 4, 5]] and singles == []
    if kind == "clique":
        assert got["families"] == 1 and got["colliding"] == 0 and got["nodes"] == 40
    if kind == "clique_minus_one":
        assert got["families"] == 1 and got["colliding"] == 1


def test_no_edges_and_bad_ids(ctx):
    got = ctx.families_of_edges([], [], np.zeros(5, np.uint32))
    assert got["nodes"] == got["families"] == got["colliding"] == 0 and got["family_off"].tolist() == [0]
    assert got["component_of"].tolist() == [0, 1, 2, 3, 4] and not got["is_node"].any()
    g = np.zeros(10, np.uint32)
    for src, dst in ([0, 10], [1, 2]), ([0, 1], [2, -1]), ([3], [1 << 30]):
        with pytest.raises(_lib.PdlError) as e:
            ctx.families_of_edges(src, dst, g)
        assert e.value.code == _lib.PDL_ERR_ARGUMENT
    lib = _lib.load()
    fam = _lib.PdlFamilies()
    one = np.zeros(1, np.int32)
    assert lib.pdl_families_of_edges(ctx._ctx, None, one.ctypes.data, 1, g.ctypes.data, 10, fam) == _lib.PDL_ERR_ARGUMENT
    assert lib.pdl_families_of_edges(ctx._ctx, one.ctypes.data, one.ctypes.data, 1, None, 10, fam) == _lib.PDL_ERR_ARGUMENT
    assert lib.pdl_families_of_edges(ctx._ctx, one.ctypes.data, one.ctypes.data, 1, g.ctypes.data, 10, None) == _lib.PDL_ERR_ARGUMENT
    got = ctx.families_of_edges([0, 1], [1, 2], g)                  # the context is as usable as before
    assert got["families"] == 1 and got["family_genes"].tolist() == [0, 1, 2] and got["colliding"] == 1


# ---- state -----------------------------------------------------------------------------------------------------------------
def _observables(nat, genomes):
    out = {"scores": [nat.generate_scores_part(g).as_dict() for g in range(genomes)],          # (the scoring pass and K-bbh run here)
           "edges": [nat.generate_edges_part(g) for g in range(genomes)]}
    out.update({"cost": nat.cost.as_dict(), "timings": nat.timings(), "dictionary": nat.dictionary(), "costs": nat.sequence_costs(),
                "genome_costs": [nat.genome_cost(g) for g in range(genomes)]})
    return out


def _assert_observables_equal(a, b):
    assert a["cost"] == b["cost"] and a["timings"] == b["timings"] and a["genome_costs"] == b["genome_costs"]
    for x, y in zip(a["dictionary"] + a["costs"], b["dictionary"] + b["costs"]):
        assert np.array_equal(x, y)
    for x, y in zip(a["scores"], b["scores"]):
        for f in H.FIELDS:
            assert np.array_equal(H.raw(x[f]), H.raw(y[f])), f
    for x, y in zip(a["edges"], b["edges"]):
        assert all(np.array_equal(H.raw(p), H.raw(q)) for p, q in zip(x, y))


def test_idempotent_and_leaves_the_context_alone(ctx):
    shape, k = CASES["paralogs_6x80x120_k3"]
    gs = make_gene_set(**shape)
    nat = _native(gs, k)
    before = _observables(nat, gs.genomes)
    a = nat.generate_families()
    other = ctx.families_of_edges([0, 1], [1, 2], np.zeros(3, np.uint32))          # another context's call in between
    assert other["families"] == 1
    mine = nat.families_of_edges([0], [1], np.zeros(2, np.uint32))                 # ... and a caller's list on this one
    assert mine["families"] == 1 and mine["sequences"] == 2
    b = nat.generate_families()
    _assert_same(a, b, "second call")
    assert a["colliding"] > 0 and nat.last_families_info["device_ms"] > 0
    _assert_observables_equal(before, _observables(nat, gs.genomes))
    nat.close()


def test_families_on_first_use_and_after_an_append():
    shape, k = CASES["paralogs_10x60x90_k3_div20"]
    gs = make_gene_set(**shape)
    first_new = int(np.searchsorted(gs.genome_of, gs.genomes - 3))              # the last three genomes join later
    off = np.asarray(gs.offsets, np.uint64)
    base = _native_arrays(k, gs.residues[:int(off[first_new])], off[:first_new + 1], gs.genome_of[:first_new])
    fam_base = base.generate_families()                                          # scoring and K-bbh run on first use
    assert fam_base["sequences"] == first_new
    base.append(gs.residues[int(off[first_new]):], off[first_new:] - off[first_new], gs.genome_of[first_new:])
    got = base.generate_families()
    whole = _native(gs, k)
    _assert_same(got, whole.generate_families(), "append")
    _check_against_script(base, gs, "append against the script")
    base.close(); whole.close()


def _native_arrays(k, residues, offsets, genome_of):
    from pandelos_amd.pangene_native import PangeneNative
    return PangeneNative.from_arrays(k, residues, offsets, genome_of)


def test_refusals_return_their_code_and_leave_the_context_usable():
    from pandelos_amd.pangene_native import PangeneNative
    shape, k = CASES["synth_5x60x80_k3"]
    gs = make_gene_set(**shape)

    def refused(nat):
        with pytest.raises(_lib.PdlError) as e:
            nat.generate_families()
        assert e.value.code == _lib.PDL_ERR_STATE, e.value

    nat = PangeneNative.open()
    refused(nat)                                                         # before a preprocess
    nat.preprocess(k, gs.residues, gs.offsets, gs.genome_of, only_complexity=True)
    refused(nat)                                                         # after only_complexity
    nat.preprocess(k, gs.residues, gs.offsets, gs.genome_of)
    want = _check_against_script(nat, gs, "after two refusals")
    nat.close()

    nat = PangeneNative.open()
    nat.set_genome_shard([0, 2])                                          # a genome shard in force
    nat.preprocess(k, gs.residues, gs.offsets, gs.genome_of)
    refused(nat)
    src, dst, _ = nat.generate_edges_part(0)                              # ... and the context goes on serving its shard
    assert len(src) > 0
    nat.close()

    nat = PangeneNative.open()                                            # low_memory batches
    blocks = dict(nat.scores_in_batches(k, gs.residues, gs.offsets, gs.genome_of, 2))
    assert len(blocks) == gs.genomes
    refused(nat)
    last = nat.generate_scores_part(gs.genomes - 1)                       # ... and the last batch is still there to be fetched
    assert H.raw(last.scores).tobytes() == H.raw(blocks[gs.genomes - 1].scores).tobytes()
    nat.close()
    assert want["families"] > 0

    lib = _lib.load()
    assert lib.pdl_compute_families(None, _lib.PdlFamilies()) == _lib.PDL_ERR_ARGUMENT
    nat = _native(gs, k)
    assert lib.pdl_compute_families(nat._ctx, None) == _lib.PDL_ERR_ARGUMENT
    nat.close()


@pytest.mark.timeout(900)
def test_refused_on_a_multi_gpu_context():
    import torch
    shape, k = CASES["synth_5x60x80_k3"]
    gs = make_gene_set(**shape)
    from pandelos_amd.pangene_native import PangeneNative
    dev = torch.device("cuda:0")
    res = torch.from_numpy(np.ascontiguousarray(gs.residues)).to(dev)
    off = torch.from_numpy(np.asarray(gs.offsets, np.uint64).view(np.int64).copy()).to(dev)
    gen = torch.from_numpy(np.asarray(gs.genome_of, np.uint32).view(np.int32).copy()).to(dev)
    torch.cuda.synchronize()
    nat = PangeneNative.open()
    ptr, records, _ = nat.dist_preprocess_begin(k, res.data_ptr(), off.data_ptr(), gen.data_ptr(), gs.genes, len(gs.residues), 1, 0,
                                                keepalive=(res, off, gen))
    post = torch.empty(max(records, 1) * 2, dtype=torch.int32, device=dev)
    nat.copy_device(post.data_ptr(), ptr, records * 8)
    nat.dist_preprocess_finish(post.data_ptr(), records, nat.run_weights, keepalive=post)
    with pytest.raises(_lib.PdlError) as e:
        nat.generate_families()
    assert e.value.code == _lib.PDL_ERR_STATE
    assert nat.dist_genome_owner().tolist() == [0] * gs.genomes           # the context is as usable as before
    nat.close()
