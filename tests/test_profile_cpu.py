"""The pan-genome profile off the device: the two references of tests/profile_cases.py against each other, the host side of
pandelos_amd/pangenome.py against them and against the committed output of the reference's example/quality.py
(tests/golden/quality, made by tests/golden/make_golden_quality.py)."""
from __future__ import annotations

import numpy as np
import pytest

from pandelos_amd import netclu
from pandelos_amd import pangenome as PG
from pandelos_amd.synth import make_gene_set
from tests import helpers as H
from tests import profile_cases as PC
from tests.test_host_net import CASES

NET, QUALITY = H.GOLDEN / "net", H.GOLDEN / "quality"
SMALL = [n for n, (f, _, _) in PC.profile_cases().items() if len(f) <= 4000]


@pytest.mark.parametrize("name", SMALL)
def test_the_two_profile_references_agree(name):
    f, g, G = PC.profile_cases()[name]
    assert PC.first_difference(PC.profile_sets(f, g, G), PC.profile_numpy(f, g, G)) is None


def test_the_two_profile_references_agree_on_a_random_set():
    f, g, G = PC.profile_cases()["random, seed 0"]
    want = PC.profile_sets(f, g, G)
    assert PC.first_difference(PC.expected_profile("random, seed 0"), want) is None
    assert want["core"] > 100 and want["unique"] > 100 and want["accessory"] > 100 and want["max_size"] > G


def test_a_relabelling_changes_the_labels_only():
    f, g, G = PC.random_labelling(100, genes=3000, genomes=9)
    base = PC.profile_numpy(f, g, G)
    for fam in (PC.relabel(f, 1), PC.relabel(f, 2, sparse=True)):
        assert (fam != f).any()
        p = PC.profile_numpy(fam, g, G)
        for n in PC.COUNTS + ("size_hist", "spread_hist", "spread_by_genome", "genome_genes", "genome_core", "genome_accessory", "genome_unique"):
            assert np.array_equal(p[n], base[n]), n
        assert sorted(p["size"].tolist()) == sorted(base["size"].tolist())
    assert not np.isin(PC.relabel(f, 2, sparse=True), f).all()            # some sparse label is no old label


@pytest.mark.parametrize("name", [n for n, ((f, _, _), o) in PC.curve_cases().items() if len(f) * len(o) <= 40000])
def test_the_curve_references_and_the_host_formulation_agree(name):
    (f, g, G), orders = PC.curve_cases()[name]
    prof, want = PC.expected_curves(name)
    assert PC.first_curve_difference(PC.curves_sets(prof, orders), want) is None
    assert PC.first_curve_difference(PG.pan_curves_host(prof, orders), want) is None


@pytest.mark.parametrize("name", sorted(PC.curve_cases()))
def test_host_curves_meet_the_identities(name):
    (f, g, G), orders = PC.curve_cases()[name]
    prof, want = PC.expected_curves(name)
    got = PG.pan_curves_host(prof, orders)
    assert PC.first_curve_difference(got, want) is None
    pan, core = got["pan"].astype(np.int64), got["core"].astype(np.int64)
    assert (pan[:, -1] == prof["families"]).all() and (core[:, -1] == prof["core"]).all() and (pan[:, 0] == core[:, 0]).all()
    assert (np.diff(pan, axis=1) >= 0).all() and (np.diff(core, axis=1) <= 0).all() and (core <= pan).all()
    first = np.array([prof["spread_by_genome"][:, o[0]].sum() for o in orders])       # the families of the first genome
    assert (pan[:, 0] == first).all()
    if name == "every family is core":
        assert (pan == prof["families"]).all() and (core == prof["families"]).all()
    if name == "no family is core":
        assert prof["core"] == 0 and (core[:, -1] == 0).all() and (core[:, 0] > 0).all()


def test_random_orders_are_seeded_permutations():
    a, b = PG.random_orders(37, 50, 1), PG.random_orders(37, 50, 1)
    assert a.dtype == np.uint32 and a.shape == (50, 37) and np.array_equal(a, b)
    assert (np.sort(a, axis=1) == np.arange(37)).all() and len({r.tobytes() for r in a}) == 50
    assert not np.array_equal(a, PG.random_orders(37, 50, 2))
    rng = np.random.Generator(np.random.PCG64(1))
    assert np.array_equal(a, rng.permuted(np.tile(np.arange(37, dtype=np.uint32), (50, 1)), axis=1))


def _fixture(name, tmp_path):
    faa = tmp_path / f"{name}.faa"
    make_gene_set(**CASES[name][0]).write_faa(faa)
    names, genome_of = netclu.read_names(faa)
    text = (NET / f"{name}.clus").read_text()
    return names, genome_of, text


@pytest.mark.parametrize("name", sorted(CASES))
def test_quality_text_equals_the_reference_scripts_output(name, tmp_path):
    names, genome_of, text = _fixture(name, tmp_path)
    gen, genome_names = PG.genome_ids(genome_of)
    fam = PG.family_of_from_clus(names, text)
    for prof in (PC.profile_numpy(fam, gen, len(genome_names)), PC.profile_sets(fam, gen, len(genome_names))):
        assert PG.quality_text(prof, genome_names) == (QUALITY / f"{name}.txt").read_text()


def test_quality_text_with_genomes_out_of_string_order_and_odd_lines():
    """Genome ids in first-seen order, the script's tables in string order; "nof reads" is half the line count."""
    fam, gen = np.array([0, 0, 2, 3, 3, 3], np.uint32), np.array([0, 1, 1, 2, 2, 0], np.uint32)
    text = PG.quality_text(PC.profile_numpy(fam, gen, 3), ["zeta", "alpha", "mid"], n_reads=7)
    lines = text.splitlines()
    assert lines[1:4] == ["nof genomes 3", "nof seqs 6", "nof reads 7"] and lines[6:9] == ["alpha 2", "mid 2", "zeta 2"]
    assert "--\talpha\tmid\tzeta\t" in lines
    assert lines[-2:] == ["1\t1\t0\t0\t", "2\t1\t1\t2\t"] and text.endswith("\t\n")        # spread 3 does not occur: no row
    assert lines[lines.index("number of sequences\tnumber of families") + 1:][:3] == ["1 1", "2 1", "3 1"]
    assert lines[lines.index("number of genomes\tnumber of families") + 1:][:2] == ["1 1", "2 2"]


def test_quality_text_dies_where_the_script_dies():
    prof = PC.profile_numpy(np.arange(5, dtype=np.uint32), np.arange(5, dtype=np.uint32) % 2, 2)
    with pytest.raises(ValueError):
        PG.quality_text(prof, ["a", "b"])
    pair = PC.profile_numpy(np.array([0, 0, 2], np.uint32), np.array([1, 1, 0], np.uint32), 2)       # two genes of one genome: the widest multi-gene family has spread 1
    lines = PG.quality_text(pair, ["a", "b"]).splitlines()
    assert lines[lines.index("number of genomes\tnumber of families") + 1:][:2] == ["1 1", "-" * 40]


@pytest.mark.parametrize("name", sorted(CASES))
def test_family_of_from_clus_round_trips_the_fixtures(name, tmp_path):
    names, genome_of, text = _fixture(name, tmp_path)
    fam = PG.family_of_from_clus(names, text)
    assert fam.dtype == np.uint32 and (fam <= np.arange(len(names))).all() and (fam[fam] == fam).all()
    gen, genome_names = PG.genome_ids(genome_of)
    prof = PC.profile_numpy(fam, gen, len(genome_names))
    lines = sorted(" ".join(names[g] for g in genes.tolist()) for genes in PG.members_by_family(prof, fam))
    assert lines == sorted(l.strip() for l in text.splitlines())
    table = PG.presence_tsv(prof, fam, names, genome_names).splitlines()
    assert table[0].split("\t") == ["family", "size", "spread"] + genome_names + ["genes"] and len(table) == prof["families"] + 1
    cols = [r.split("\t") for r in table[1:]]
    assert sorted(c[-1] for c in cols) == lines
    assert all(int(c[1]) == sum(map(int, c[3:-1])) == len(c[-1].split(" ")) and int(c[2]) == sum(x != "0" for x in c[3:-1]) for c in cols)


def test_family_of_from_clus_refusals_and_missing_genes():
    names = ["a", "b", "c", "d"]
    assert PG.family_of_from_clus(names, "c b\nd \n").tolist() == [0, 1, 1, 3]          # `a` is not named: alone
    for bad in ("a b\nb c\n", "a a\n", "a x\n"):
        with pytest.raises(ValueError):
            PG.family_of_from_clus(names, bad)
    with pytest.raises(ValueError):
        PG.family_of_from_clus(["a", "a"], "a\n")


def test_curves_tsv():
    curves = {"pan": np.array([[2, 3, 5], [1, 4, 5]], np.uint32), "core": np.array([[2, 1, 1], [1, 1, 1]], np.uint32)}
    lines = PG.curves_tsv(curves).splitlines()
    assert lines[0].split("\t") == ["genomes", "pan_mean", "pan_min", "pan_max", "core_mean", "core_min", "core_max", "new_mean", "new_min", "new_max"]
    assert lines[1] == "1\t1.500\t1\t2\t1.500\t1\t2\t1.500\t1\t2" and lines[2] == "2\t3.500\t3\t4\t1.000\t1\t1\t2.000\t1\t3"
    assert lines[3] == "3\t5.000\t5\t5\t1.000\t1\t1\t1.500\t1\t2"
