"""K-split on the device (pdl_split_first_level, pandelos_amd/csrc/pdl_split.h): the removed-edge sequences must be exactly
those of the flat restatement of the contract (tests/split_cases.py; test_split_cpu.py holds it against netclu's loop)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from pandelos_amd import _lib, netclu
from pandelos_amd import families as FAM
from pandelos_amd.synth import make_gene_set
from tests import helpers as H
from tests import split_cases as SC
from tests.test_host_net import CASES

pytestmark = pytest.mark.gpu
NET, SPLIT = H.GOLDEN / "net", H.GOLDEN / "split"
PARALOGS = ("paralogs_6x80x120_k3", "paralogs_10x60x90_k3_div20")
COMMUNITIES = ("community_100", "community_200", "community_mixed")


@pytest.fixture(scope="module")
def ctx():
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.open()                        # no preprocess: pdl_split_first_level needs none
    yield nat
    nat.close()


def _check(ctx, graphs, label):
    got = ctx.split_first_level(graphs)
    assert len(got) == len(graphs)
    for j, (g, rem) in enumerate(zip(graphs, got)):
        assert rem == SC.flat_on_graph(g), f"{label}, graph {j} ({len(g)} nodes)"
    return got


@pytest.mark.parametrize("name", sorted(SC.small_graphs()))
def test_small_graphs(name, ctx):
    g = SC.small_graphs()[name]
    got = _check(ctx, [g], name)[0]
    assert (len(got) == 0) == (name == "one node")
    if name == "two triangles on a bridge":
        assert got == [(2, 3)]
    if name == "triangle":
        assert got[0] == netclu.edge_list(g)[0]                  # three-way tie: the first edge
    info = ctx.last_split_info
    assert info["graphs"] == 1 and info["nodes"] == len(g) and info["edges"] == len(netclu.edge_list(g)) and info["removals"] == len(got) == info["rounds"]


@pytest.mark.parametrize("name", sorted(SC.chunk_edge_graphs()))
def test_chunk_edges(name, ctx):
    _check(ctx, [SC.chunk_edge_graphs()[name]], name)


BEYOND_LDS = ("two K56 on a bridge", "two K56 on two paths", "two K56 on three paths")


@pytest.mark.parametrize("name", BEYOND_LDS)
def test_adjacency_that_does_not_fit_lds(name, ctx):
    """The kernel's second storage path: removed marks in the workgroup's scratch, offsets and edge ids from global memory."""
    g, want = SC.beyond_lds_graphs()[name]
    assert SC.lds_words(g) > SC.LDS_WORDS > SC.lds_words(SC.two_cliques(55, [0]))
    assert ctx.split_first_level([g]) == [want]
    assert want == [(0, 56)] if name == "two K56 on a bridge" else len(want) >= 2
    # ... behind graphs that do fit, so that its first node, slot and edge are not the arrays' first: the offsets' base is used
    small = SC.small_graphs()
    front = [small["Q4"], SC.random_graph(3)]
    assert ctx.split_first_level(front + [g, small["K4"]]) == [SC.flat_on_graph(h) for h in front] + [want, SC.flat_on_graph(small["K4"])]


def test_all_random_graphs_in_one_call(ctx):
    graphs, want = SC.random_expected()
    got = ctx.split_first_level(graphs)
    bad = [s for s, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, f"seeds {bad[:10]} of {len(bad)} differ"
    info = ctx.last_split_info
    assert info["graphs"] == len(graphs) and info["chunks"] == 1 and info["removals"] == sum(len(w) for w in want) and info["device_ms"] > 0


def test_random_graphs_cut_into_chunks(ctx):
    """A budget of exactly the largest graph's scratch cuts the 400 into many launches; the largest has a launch to itself."""
    graphs, want = SC.random_expected()
    need = sorted(_scratch(g) for g in graphs)
    try:
        ctx.set_option("split_scratch_bytes", need[-1])
        got = ctx.split_first_level(graphs)
        chunks = ctx.last_split_info["chunks"]
        one = ctx.split_first_level([graphs[0], max(graphs, key=_scratch), max(graphs, key=_scratch), graphs[1]])
        assert ctx.last_split_info["chunks"] == 4
    finally:
        ctx.set_option("split_scratch_bytes", 1 << 30)
    assert got == want and chunks > 10
    big = want[max(range(len(graphs)), key=lambda j: _scratch(graphs[j]))]
    assert one == [want[0], big, big, want[1]]


def _scratch(g):
    """split_scratch_bytes of pdl_split.h."""
    n, m, lanes = len(g), len(netclu.edge_list(g)), 256
    return 0 if m == 0 else (8 * (m + lanes * m + 2 * lanes * n) + 4 * (2 * lanes * n + n + 2 * m) + 255) & ~255


def test_one_graph_twice_and_smallest_beside_largest(ctx):
    small, big = SC.small_graphs(), SC.chunk_edge_graphs()
    _check(ctx, [small["Q4"], small["Q4"]], "twice")
    _check(ctx, [small["one node"], big["cycle of 257"], small["one edge"]], "side by side")


def _raw(ctx, node_off, adj_off, adj, n_graphs=None):
    no, ao, ad = np.asarray(node_off, np.uint64), np.asarray(adj_off, np.uint64), np.asarray(adj, np.uint32)
    s = _lib.PdlSplit()
    rc = ctx._lib.pdl_split_first_level(ctx._ctx, len(no) - 1 if n_graphs is None else n_graphs, no.ctypes.data, ao.ctypes.data, ad.ctypes.data, C.byref(s))
    assert rc == _lib.PDL_OK or (not s.removed_off and not s.removed_u and s.removals == 0)
    ctx._lib.pdl_free_split(C.byref(s))
    return rc


def test_malformed_input_is_refused_and_the_next_call_is_right(ctx):
    (no, ao, ad), want = SC.legal_packing()
    for name, packing in SC.malformed_packings().items():
        assert _raw(ctx, *packing) == _lib.PDL_ERR_ARGUMENT, name
        assert ctx.split_packed(no, ao, ad) == want, f"behind {name}"
    lib, s = ctx._lib, _lib.PdlSplit()
    assert _raw(ctx, no, ao, ad, n_graphs=0) == _lib.PDL_ERR_ARGUMENT
    assert lib.pdl_split_first_level(ctx._ctx, 2, None, ao.ctypes.data, ad.ctypes.data, C.byref(s)) == _lib.PDL_ERR_ARGUMENT
    assert lib.pdl_split_first_level(ctx._ctx, 2, no.ctypes.data, None, ad.ctypes.data, C.byref(s)) == _lib.PDL_ERR_ARGUMENT
    assert lib.pdl_split_first_level(ctx._ctx, 2, no.ctypes.data, ao.ctypes.data, None, C.byref(s)) == _lib.PDL_ERR_ARGUMENT
    assert lib.pdl_split_first_level(ctx._ctx, 2, no.ctypes.data, ao.ctypes.data, ad.ctypes.data, None) == _lib.PDL_ERR_ARGUMENT
    assert lib.pdl_split_first_level(None, 2, no.ctypes.data, ao.ctypes.data, ad.ctypes.data, C.byref(s)) == _lib.PDL_ERR_ARGUMENT
    assert ctx.split_packed(no, ao, ad) == want


def test_a_graph_over_a_tiny_budget_is_unsupported(ctx):
    (no, ao, ad), want = SC.legal_packing()
    try:
        ctx.set_option("split_scratch_bytes", 1024)
        with pytest.raises(_lib.PdlError) as e:
            ctx.split_packed(no, ao, ad)
        assert e.value.code == _lib.PDL_ERR_UNSUPPORTED and "split_scratch_bytes" in str(e.value)
        with pytest.raises(_lib.PdlError) as e:
            ctx.set_option("split_scratch_bytes", 0)
        assert e.value.code == _lib.PDL_ERR_ARGUMENT
    finally:
        ctx.set_option("split_scratch_bytes", 1 << 30)
    assert ctx.split_packed(no, ao, ad) == want


def test_leaves_a_scored_context_alone_and_answers_twice_alike():
    from tests.test_gpu_families import _assert_observables_equal, _assert_same, _native, _observables
    shape, k = CASES["paralogs_6x80x120_k3"]
    gs = make_gene_set(**shape)
    nat = _native(gs, k)
    fam = nat.generate_families()
    before = _observables(nat, gs.genomes)
    graphs = [SC.small_graphs()["Q3"], SC.random_graph(5)]
    a = nat.split_first_level(graphs)
    b = nat.split_first_level(graphs)
    assert a == b == [SC.flat_on_graph(g) for g in graphs] and nat.last_split_info["device_ms"] > 0
    _assert_observables_equal(before, _observables(nat, gs.genomes))
    _assert_same(nat.generate_families(), fam, "families behind the split")
    nat.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PARALOGS)
def test_command_writes_the_paralog_fixtures_either_way(name, tmp_path, capsys):
    shape, k = CASES[name]
    faa, dev, host = tmp_path / "in.faa", tmp_path / "dev.clus", tmp_path / "host.clus"
    make_gene_set(**shape).write_faa(faa)
    assert FAM.main(["-i", str(faa), "-k", str(k), "-o", str(dev)]) == 0
    assert "K-split:" in capsys.readouterr().out
    info = FAM.last_split_info                                   # the command's last call, and its totals
    assert info["removals"] > 0 and info["totals"]["removals"] >= info["removals"] and info["totals"]["calls"] > 1
    assert info["totals"]["graphs"] >= {PARALOGS[0]: 51, PARALOGS[1]: 68}[name]
    assert FAM.main(["-i", str(faa), "-k", str(k), "-o", str(host), "--host-split"]) == 0
    assert "K-split:" not in capsys.readouterr().out and FAM.last_split_info is None
    want = (NET / f"{name}.clus").read_text()
    assert dev.read_text() == want and host.read_bytes() == dev.read_bytes()


@pytest.mark.parametrize("name", COMMUNITIES)
def test_command_writes_the_community_fixtures(name, tmp_path):
    out = tmp_path / "out.clus"
    assert FAM.main(["-i", str(SPLIT / f"{name}.faa"), "--from-net", str(SPLIT / f"{name}.net"), "-o", str(out)]) == 0
    assert out.read_text() == (SPLIT / f"{name}.clus").read_text()
    assert FAM.last_split_info["removals"] > 0 and FAM.last_split_info["totals"]["removals"] >= FAM.last_split_info["removals"]


def test_command_from_a_net_with_the_host_split(tmp_path):
    name = "community_100"                                       # (0.6 s of the host's loop)
    dev, host = tmp_path / "dev.clus", tmp_path / "host.clus"
    args = ["-i", str(SPLIT / f"{name}.faa"), "--from-net", str(SPLIT / f"{name}.net")]
    assert FAM.main(args + ["-o", str(dev)]) == 0 and FAM.last_split_info["removals"] > 0
    assert FAM.main(args + ["-o", str(host), "--host-split"]) == 0 and FAM.last_split_info is None
    assert host.read_bytes() == dev.read_bytes() == (SPLIT / f"{name}.clus").read_bytes()
    with pytest.raises(SystemExit):                              # without a .net the command still asks for k
        FAM.main(["-i", str(SPLIT / f"{name}.faa"), "-o", str(dev)])


def test_split_totals_of_the_families_road(ctx, tmp_path):
    name = PARALOGS[1]
    make_gene_set(**CASES[name][0]).write_faa(tmp_path / "in.faa")
    names, genome_of = netclu.read_names(tmp_path / "in.faa")
    src, dst = netclu.read_net_edges(NET / f"{name}.net")
    ids = {}
    fam = ctx.families_of_edges(src, dst, np.array([ids.setdefault(g, len(ids)) for g in genome_of], np.uint32))
    splitter = FAM.DeviceSplitter(ctx)
    fams, singles = netclu.families_from_components(names, genome_of, fam, src, dst, net_ordered=True, first_level=splitter)
    assert netclu.clus_text(names, fams, singles) == (NET / f"{name}.clus").read_text()
    assert ctx.last_split_info["removals"] > 0 and splitter.totals["removals"] >= ctx.last_split_info["removals"]
    assert splitter.totals["graphs"] >= fam["colliding"] == 68


@pytest.mark.timeout(900)
def test_families_on_random_sets_either_splitter(ctx):
    """The 60 seeds of test_gpu_families.py's random sets (every second with paralogs): the device splitter's families are the
    host splitter's."""
    from tests.test_gpu_families import SEEDS, _native, random_shape
    removals = 0
    for seed in range(SEEDS):
        shape, k = random_shape(seed)
        gs = make_gene_set(**shape)
        nat = _native(gs, k)
        fam = nat.generate_families()
        if fam["colliding"]:
            src, dst, _ = FAM.gather_edges(nat, gs.genomes)
            names, gen = [str(i) for i in range(gs.genes)], gs.genome_of.tolist()
            splitter = FAM.DeviceSplitter(ctx)
            dev = netclu.families_from_components(names, gen, fam, src, dst, first_level=splitter)
            assert dev == netclu.families_from_components(names, gen, fam, src, dst), f"seed {seed} {shape}"
            removals += splitter.totals["removals"]
        nat.close()
    assert removals > 0
