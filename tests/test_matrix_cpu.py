"""The genome-by-genome shared-family matrices off the device: the two references of tests/matrix_cases.py against each other and
against pangenome.genome_matrix_host, the identities the matrices meet, the unary-plane identity the kernel rests on
(popcounts over matrix_cases.stacked_bits), every case on the side of the kernel's constants its name says, and the host side of
pandelos_amd/pangenome.py (distances, pair pan / core, the table, the command with the host formulation in the device's place)."""
from __future__ import annotations

import numpy as np
import pytest

from pandelos_amd import netclu
from pandelos_amd import pangenome as PG
from pandelos_amd.synth import make_gene_set
from tests import helpers as H
from tests import matrix_cases as MC
from tests import profile_cases as PC
from tests.test_host_net import CASES

NET = H.GOLDEN / "net"
PARALOGS = ("paralogs_6x80x120_k3", "paralogs_10x60x90_k3_div20")
NAMES = list(MC.matrix_cases())


@pytest.mark.parametrize("name", [n for n in NAMES if MC.small(n)])
def test_the_two_references_agree(name):
    f, g, G = MC.matrix_cases()[name]
    assert MC.first_difference(MC.matrices_sets(f, g, G), MC.expected(name)[1]) is None


@pytest.mark.parametrize("name", NAMES)
def test_host_formulation_and_identities(name):
    f, g, G = MC.matrix_cases()[name]
    prof, want = MC.expected(name)
    got = PG.genome_matrix_host(prof)
    assert got["shared"].dtype == np.uint32 and got["shared"].shape == (G, G)
    assert MC.first_difference(got, want) is None
    s, c = got["shared"].astype(np.int64), got["shared_copies"].astype(np.int64)
    assert (s == s.T).all() and (c == c.T).all() and (s <= c).all()
    assert (np.diag(s) == prof["spread_by_genome"].astype(np.int64).sum(axis=0)).all()
    assert (np.diag(c) == prof["genome_genes"]).all()
    table = PG.copies_matrix(prof)
    assert table.shape == (prof["families"], G) and (table.sum(axis=1) == prof["size"]).all() and ((table > 0) == PG.presence_matrix(prof)).all()


@pytest.mark.parametrize("name", [n for n in NAMES if MC.small(n) or n.startswith("k-split")])
def test_popcounts_over_the_stacked_bits_reproduce_both_matrices(name):
    """min(a, b) = sum over t >= 1 of [a >= t][b >= t]: the products of the bit rows are the matrices."""
    prof, want = MC.expected(name)
    lay = MC.layout(prof)
    bits = MC.stacked_bits(prof).astype(np.int64)
    assert bits.shape[1] == lay["L"] and not bits[:, lay["F"]:lay["P"]].any()           # (the columns between F and P stay clear)
    got = {"shared": bits[:, :lay["P"]] @ bits[:, :lay["P"]].T, "shared_copies": bits @ bits.T}
    assert MC.first_difference(got, want) is None
    assert lay["E"] <= prof["n_sequences"] - prof["families"] and lay["L"] <= prof["n_sequences"] + 63


@pytest.mark.parametrize("name", [n for n in NAMES if MC.matrix_cases()[n][2] <= 130 and len(MC.matrix_cases()[n][0]) <= 4000])
def test_pair_pan_core_equals_the_curves_at_the_second_genome(name):
    prof, want = MC.expected(name)
    G = prof["n_genomes"]
    pan2, core2 = PG.pair_pan_core(want["shared"])
    pairs = [(g, h) for g in range(G) for h in range(G) if g != h][::max(1, G * G // 60)]
    if not pairs:
        return
    orders = np.array([[g, h] + [x for x in range(G) if x not in (g, h)] for g, h in pairs], np.uint32)
    curves = PG.pan_curves_host(prof, orders)
    assert curves["pan"][:, 1].tolist() == [int(pan2[g, h]) for g, h in pairs]
    assert curves["core"][:, 1].tolist() == [int(core2[g, h]) for g, h in pairs]


def test_every_case_lies_where_its_name_says():
    lay = {n: MC.layout(MC.expected(n)[0]) for n in NAMES}
    G = {n: MC.matrix_cases()[n][2] for n in NAMES}
    assert [G[f"G = {g}"] for g in MC.G_EDGES] == list(MC.G_EDGES) and {g % MC.TILE for g in MC.G_EDGES} == {MC.TILE - 1, 0, 1}
    assert G["1025 genomes"] == 1025 and -(-1025 // MC.TILE) == 17 and 250 <= lay["1025 genomes"]["F"] <= 300
    for F in MC.F_EDGES:
        a, b = lay[f"F = {F}, single copies"], lay[f"F = {F}, with extras"]
        assert a["F"] == b["F"] == F and a["E"] == 0 and b["E"] > 0 and a["P"] - F == (-F) % MC.WORD
    assert {(-F) % MC.WORD for F in MC.F_EDGES} >= {0, 1, 63}
    assert lay["all singletons"]["E"] == 0 and lay["one family of everything"]["F"] == 1
    prof = MC.expected("a genome without a gene")[0]
    assert prof["genome_genes"][2] == 0
    assert MC.expected("copies (3, 1, 2)")[0]["copies"][:3].tolist() == [3, 1, 2]
    big = lay["200 copies in one genome"]
    assert big["extra"][0] == 199 and (big["P"] + 198) // MC.WORD - big["P"] // MC.WORD == 3        # its run lies in four words
    edge = lay["70 copies from the last bit of a word"]
    assert edge["extra"][1] == 69 and (edge["P"] + edge["extra_off"][1]) % MC.WORD == MC.WORD - 1
    assert MC.expected("copies >= 2 everywhere")[0]["copies"].min() >= 2 and MC.expected("copies >= 2 everywhere")[0]["core"] == 70
    # slabs: three and more, one cut inside the extras; one word each
    prof = MC.expected("slabs")[0]
    plan, pw = MC.slab_plan(prof, MC.SLAB_BYTES), lay["slabs"]["P"] // MC.WORD
    assert len(plan) >= 3 and sum(w0 >= pw for w0, _ in plan) >= 2 and all(w1 - w0 <= 3 and (w1 <= pw or w0 >= pw) for w0, w1 in plan)
    assert MC.slab_plan(prof, 1) == [(w, w + 1) for w in range(lay["slabs"]["W"])] and len(MC.slab_plan(prof)) == 2
    # k-splits: one pair of tiles, so the count follows from the slab's words alone
    for name in ("k-split, 64 genomes", "k-split, short last part"):
        assert G[name] == MC.TILE
        w0, w1 = MC.slab_plan(MC.expected(name)[0])[0]
        assert MC.split_plan(w1 - w0, G[name], cus=64) == MC.split_plan(w1 - w0, G[name], cus=304) and MC.split_plan(w1 - w0, G[name])[0] > 1
    assert 18000 <= len(MC.matrix_cases()["k-split, 64 genomes"][0]) <= 24000
    splits, per = MC.split_plan(lay["k-split, short last part"]["P"] // MC.WORD, MC.TILE)
    assert 0 < lay["k-split, short last part"]["P"] // MC.WORD - (splits - 1) * per < MC.KSTEP
    for g in (7, 64, 130):
        assert G[f"random, {g} genomes"] == g and 20000 <= len(MC.matrix_cases()[f"random, {g} genomes"][0]) <= 20000 + 4 * g


def test_jaccard_distance():
    m = np.array([[3, 3, 0, 0], [3, 3, 0, 0], [0, 0, 2, 0], [0, 0, 0, 0]], np.uint32)       # 0 = 1; 2 disjoint from both; 3 is empty
    d = PG.jaccard_distance(m)
    assert d.dtype == np.float64 and (d == d.T).all() and (np.diag(d) == 0.0).all()
    assert d[0, 1] == 0.0 and d[0, 2] == 1.0 and d[2, 3] == 1.0 and d[3, 3] == 0.0
    prof, want = MC.expected("copies (3, 1, 2)")
    for m in want.values():
        m = m.astype(np.int64)
        d = PG.jaccard_distance(m)
        for g in range(3):
            for h in range(3):
                assert d[g, h] == 1.0 - m[g, h] / (m[g, g] + m[h, h] - m[g, h])
    pan2, core2 = PG.pair_pan_core(want["shared"])
    assert (core2 == want["shared"]).all() and (np.diag(pan2) == np.diag(want["shared"])).all()
    assert (PG.jaccard_distance(want["shared"]) == 1.0 - core2 / pan2).all()


def _parse(text):
    rows = [line.split("\t") for line in text.splitlines()]
    assert rows[0][0] == "" and [r[0] for r in rows[1:]] == rows[0][1:]
    return rows[0][1:], [r[1:] for r in rows[1:]]


def test_matrix_tsv_round_trips():
    names = ["b", "a c", "z"]
    m = np.array([[5, 0, 4000000000], [0, 1, 2], [4000000000, 2, 7]], np.uint32)
    got_names, cells = _parse(PG.matrix_tsv(m, names))
    assert got_names == names and np.array_equal(np.array(cells, np.uint64), m) and PG.matrix_tsv(m, names).endswith("\t2\t7\n")
    d = PG.jaccard_distance(np.array([[3, 1, 0], [1, 2, 0], [0, 0, 7]]))
    _, cells = _parse(PG.matrix_tsv(d, names))
    assert np.array_equal(np.array([[float(x) for x in r] for r in cells]), d) and cells[0][1] == repr(0.75) and cells[0][0] == "0.0"
    with pytest.raises(ValueError):
        PG.matrix_tsv(m, names[:2])


class _HostContext:
    """PangeneNative for the command, with the references and the host formulation where the device calls are."""
    def family_profile(self, family_of, genome_of, n_genomes):
        self.last_profile_info = {"device_ms": 0.0}
        return PC.profile_numpy(family_of, genome_of, n_genomes)

    def genome_matrix(self, profile):
        return {**PG.genome_matrix_host(profile), "levels": MC.layout(profile)["L"], "device_ms": 0.0}

    def close(self):
        pass


@pytest.mark.parametrize("name", PARALOGS)
def test_command_writes_tables_that_parse_back_to_the_reference(name, tmp_path, monkeypatch, capsys):
    from pandelos_amd import pangene_native
    monkeypatch.setattr(pangene_native.PangeneNative, "open", classmethod(lambda cls, *a, **k: _HostContext()))
    faa = tmp_path / "in.faa"
    make_gene_set(**CASES[name][0]).write_faa(faa)
    paths = {n: tmp_path / f"{n}.tsv" for n in ("shared", "shared-copies", "distance", "distance-copies")}
    argv = ["-i", str(faa), "--clus", str(NET / f"{name}.clus")]
    for n, p in paths.items():
        argv += [f"--{n}", str(p)]
    assert PG.main(argv) == 0 and "bit columns" in capsys.readouterr().out
    names, genome_of = netclu.read_names(faa)
    gen, genome_names = PG.genome_ids(genome_of)
    fam = PG.family_of_from_clus(names, (NET / f"{name}.clus").read_text())
    want = MC.matrices_numpy(fam, gen, len(genome_names))
    assert MC.first_difference(MC.matrices_sets(fam, gen, len(genome_names)), want) is None
    for n, key in (("shared", "shared"), ("shared-copies", "shared_copies")):
        got_names, cells = _parse(paths[n].read_text())
        assert got_names == genome_names and np.array_equal(np.array(cells, np.int64), want[key])
        _, cells = _parse(paths["distance" + n[6:]].read_text())
        assert np.array_equal(np.array([[float(x) for x in r] for r in cells]), PG.jaccard_distance(want[key]))
    assert (want["shared_copies"] != want["shared"]).any()              # (paralogs: copies count for something here)
