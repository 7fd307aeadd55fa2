"""The genome-by-genome shared-family matrices on the device (pdl_genome_matrix; pandelos_amd/csrc/pdl_matrix.h): every element of
both matrices equals the references of tests/matrix_cases.py (test_matrix_cpu.py holds those against each other), a failure names
the first wrong (g, h), every refusal has its code and leaves `out` zeroed, and the call touches nothing of the context it runs
on.  Every case runs behind a call on another set."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from pandelos_amd import _lib
from pandelos_amd import pangenome as PG
from pandelos_amd.synth import make_gene_set
from tests import helpers as H
from tests import matrix_cases as MC
from tests import profile_cases as PC
from tests.test_host_net import CASES

pytestmark = pytest.mark.gpu
NET = H.GOLDEN / "net"
PARALOGS = ("paralogs_6x80x120_k3", "paralogs_10x60x90_k3_div20")


@pytest.fixture(scope="module")
def ctx():
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.open()                        # no preprocess: the call needs none
    yield nat
    nat.close()


@pytest.fixture(scope="module")
def other():
    """Another set's profile: 130 genomes, copies up to 5, more levels than most cases have."""
    f, g, G = MC.random_copies(130, 900, seed=77, density=0.6, max_copies=5, p_multi=0.5)
    return PC.profile_numpy(f, g, G)


def _poison(ctx, other):
    """Leaves the context's work buffers full of another set's extras, offsets, bit rows and sums: a kernel that trusted a buffer
    it should have cleared or written shows in the call behind this one."""
    ctx.genome_matrix(other)


def _check_info(got, prof, slab_bytes=MC.DEFAULT_SLAB_BYTES):
    lay = MC.layout(prof)
    assert (got["n_genomes"], got["families"], got["incidences"]) == (prof["n_genomes"], prof["families"], prof["incidences"])
    assert got["levels"] == lay["L"] and got["slabs"] == len(MC.slab_plan(prof, slab_bytes)) and got["splits"] >= 1 and got["device_ms"] > 0


@pytest.mark.parametrize("name", list(MC.matrix_cases()))
def test_matrix_cases(name, ctx, other):
    prof, want = MC.expected(name)
    _poison(ctx, other)
    got = ctx.genome_matrix(prof)
    assert MC.first_difference(got, want) is None, name
    assert got["shared"].dtype == np.uint32 and got["shared"].shape == (prof["n_genomes"], prof["n_genomes"])
    _check_info(got, prof)
    assert ctx.last_matrix_info == {n: got[n] for n in ("n_genomes", "families", "incidences", "levels", "slabs", "splits", "device_ms")}
    assert (np.diag(got["shared_copies"]) == prof["genome_genes"]).all()
    if name == "a genome without a gene":
        assert not got["shared"][2].any() and not got["shared"][:, 2].any() and not got["shared_copies"][2].any() and not got["shared_copies"][:, 2].any()


def test_a_profile_made_on_the_device_and_twice_alike(ctx, other):
    f, g, G = MC.matrix_cases()["random, 64 genomes"]
    prof = ctx.family_profile(f, g, G)
    a, b = ctx.genome_matrix(prof), ctx.genome_matrix(prof)
    assert MC.first_difference(a, MC.expected("random, 64 genomes")[1]) is None and MC.first_difference(a, b) is None


@pytest.mark.parametrize("slab_bytes", [MC.SLAB_BYTES, 1])
def test_slabs(slab_bytes, ctx, other):
    """Three words of the ten genomes per slab: two presence slabs, and a cut inside the extras; then a word per slab."""
    prof, want = MC.expected("slabs")
    plan = MC.slab_plan(prof, slab_bytes)
    assert len(plan) >= 3
    default = ctx.genome_matrix(prof)
    ctx.set_option("matrix_slab_bytes", slab_bytes)
    try:
        _poison(ctx, other)
        got = ctx.genome_matrix(prof)
    finally:
        ctx.set_option("matrix_slab_bytes", MC.DEFAULT_SLAB_BYTES)
    assert MC.first_difference(got, want) is None and MC.first_difference(got, default) is None
    _check_info(got, prof, slab_bytes)
    assert got["slabs"] == len(plan) and default["slabs"] == 2
    with pytest.raises(_lib.PdlError) as e:
        ctx.set_option("matrix_slab_bytes", 0)
    assert e.value.code == _lib.PDL_ERR_ARGUMENT


@pytest.mark.parametrize("name", ["k-split, 64 genomes", "k-split, short last part"])
def test_k_splits(name, ctx, other):
    prof, want = MC.expected(name)
    _poison(ctx, other)
    got = ctx.genome_matrix(prof)
    assert MC.first_difference(got, want) is None
    w0, w1 = MC.slab_plan(prof)[0]
    assert got["splits"] == MC.split_plan(w1 - w0, prof["n_genomes"])[0] > 1


def test_pairs_agree_with_the_curves_at_the_second_genome(ctx):
    f, g, G = MC.matrix_cases()["9 genomes"]
    prof = MC.expected("9 genomes")[0]
    pan2, core2 = PG.pair_pan_core(ctx.genome_matrix(prof)["shared"])
    pairs = [(a, b) for a in range(G) for b in range(G) if a != b]
    orders = np.array([[a, b] + [x for x in range(G) if x not in (a, b)] for a, b in pairs], np.uint32)
    curves = ctx.pan_curves(prof, orders)
    assert curves["pan"][:, 1].tolist() == [int(pan2[a, b]) for a, b in pairs]
    assert curves["core"][:, 1].tolist() == [int(core2[a, b]) for a, b in pairs]
    assert (curves["pan"][:, 0] == np.diag(core2)[[a for a, _ in pairs]]).all()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
FIELDS = ("size", "spread", "genome_off", "genomes", "copies")


def _raw_matrix(ctx, prof, out=True, handle=True, **changed):
    keep = {n: np.ascontiguousarray(changed.get(n, prof[n]), dtype=np.uint32) for n in FIELDS if changed.get(n, 0) is not None}
    p = _lib.PdlProfile(**{n: int(changed.get(n, prof[n])) for n in ("n_sequences", "n_genomes", "families", "incidences", "core")})
    for n, a in keep.items():                         # (an array that is left out stays a NULL pointer)
        setattr(p, n, a.ctypes.data_as(_lib._pu32))
    m = _lib.PdlGenomeMatrix(n_genomes=7, levels=9, slabs=3, device_ms=1.5)            # (what a refusal has to zero)
    rc = ctx._lib.pdl_genome_matrix(ctx._ctx if handle else None, C.byref(p) if changed.get("profile", 0) is not None else None, C.byref(m) if out else None)
    msg = ctx._lib.pdl_last_error(ctx._ctx).decode()
    if rc != _lib.PDL_OK and out:
        assert not m.shared and not m.shared_copies and bytes(m) == bytes(C.sizeof(m)), "out is not zeroed"
    ctx._lib.pdl_free_genome_matrix(C.byref(m))
    return rc, msg


def _contradictions(prof):
    """name -> the changed fields: what the shared check refuses for both calls, then what it refuses for the matrices alone."""
    G = prof["n_genomes"]
    off, gen, spread, copies, size = (prof[n] for n in ("genome_off", "genomes", "spread", "copies", "size"))
    wide = int(np.argmax(spread >= 2))
    swapped = gen.copy(); swapped[off[wide]:off[wide] + 2] = swapped[off[wide]:off[wide] + 2][::-1]
    twice = gen.copy(); twice[off[wide] + 1] = twice[off[wide]]
    outside = gen.copy(); outside[off[wide + 1] - 1] = G
    shifted = off.copy(); shifted[0] = 1
    short = off.copy(); short[-1] -= 1
    empty = off.copy(); empty[wide + 1] = empty[wide]
    other_spread = spread.copy(); other_spread[wide] += 1
    both = dict(families=dict(families=prof["families"] - 1), no_family=dict(families=0), no_genome=dict(n_genomes=0),
                incidences=dict(incidences=prof["incidences"] + 1), core=dict(core=prof["core"] + 1), fewer_genomes=dict(n_genomes=G - 1),
                descending=dict(genomes=swapped), twice=dict(genomes=twice), outside=dict(genomes=outside), shifted=dict(genome_off=shifted),
                short=dict(genome_off=short), empty_row=dict(genome_off=empty), spread=dict(spread=other_spread),
                null_off=dict(genome_off=None), null_genomes=dict(genomes=None), null_spread=dict(spread=None))
    zero = copies.copy(); zero[off[wide]] = 0
    more = copies.copy(); more[off[wide]] += 1
    bigger = size.copy(); bigger[wide] += 1
    moved = size.copy(); moved[wide] += 1; moved_copies = copies.copy(); moved_copies[off[wide]] += 1      # rows add up, the genes do not
    own = dict(zero_copies=dict(copies=zero), copies_above_size=dict(copies=more), size_above_copies=dict(size=bigger),
               genes=dict(size=moved, copies=moved_copies), fewer_genes=dict(n_sequences=prof["n_sequences"] - 1),
               null_copies=dict(copies=None), null_size=dict(size=None))
    return both, own


def test_refusals_and_the_next_call_is_right(ctx):
    prof, want = MC.expected("9 genomes")
    assert _raw_matrix(ctx, prof)[0] == _lib.PDL_OK
    assert _raw_matrix(ctx, prof, profile=None)[0] == _lib.PDL_ERR_ARGUMENT
    assert _raw_matrix(ctx, prof, out=False)[0] == _lib.PDL_ERR_ARGUMENT
    assert _raw_matrix(ctx, prof, handle=False)[0] == _lib.PDL_ERR_ARGUMENT
    both, own = _contradictions(prof)
    for name, changed in {**both, **own}.items():
        rc, msg = _raw_matrix(ctx, prof, **changed)
        assert rc == _lib.PDL_ERR_ARGUMENT and msg.startswith("pdl_genome_matrix: "), (name, rc, msg)
        assert MC.first_difference(ctx.genome_matrix(prof), want) is None, f"behind {name}"
    assert "0 copies" in _raw_matrix(ctx, prof, **own["zero_copies"])[1]
    assert "add up to" in _raw_matrix(ctx, prof, **own["copies_above_size"])[1] and "genes" in _raw_matrix(ctx, prof, **own["genes"])[1]


def _one_core_family(G):
    """The fields both calls read of the profile of one family with a gene in every one of G genomes."""
    one = np.ones(1, np.uint32)
    return dict(n_sequences=G, n_genomes=G, families=1, incidences=G, core=1, size=one * G, spread=one * G,
                genome_off=np.array([0, G], np.uint32), genomes=np.arange(G, dtype=np.uint32), copies=np.ones(G, np.uint32))


def test_8193_genomes_are_refused_on_the_host(ctx):
    G = _lib.PDL_PROFILE_MAX_GENOMES + 1
    prof = _one_core_family(G)
    assert MC.first_difference(ctx.genome_matrix(_one_core_family(70)), {n: np.ones((70, 70), np.uint32) for n in ("shared", "shared_copies")}) is None
    rc, msg = _raw_matrix(ctx, prof)
    assert rc == _lib.PDL_ERR_UNSUPPORTED and "8193 genomes" in msg and "8192" in msg
    with pytest.raises(_lib.PdlError) as e:
        ctx.genome_matrix(prof)
    assert e.value.code == _lib.PDL_ERR_UNSUPPORTED
    small, want = MC.expected("two genomes")
    assert MC.first_difference(ctx.genome_matrix(small), want) is None


def test_the_curves_refusals_read_as_before(ctx):
    """pdl_pan_curves' check of the profile is the function pdl_genome_matrix uses: its codes and messages, character for
    character, as they were before the two shared it."""
    from tests.test_gpu_profile import _raw_curves
    prof, _ = MC.expected("9 genomes")
    G, F, Z = prof["n_genomes"], prof["families"], prof["incidences"]
    off, gen, spread = prof["genome_off"], prof["genomes"], prof["spread"]
    orders = PC.order_set(G, 3, 1)
    both, own = _contradictions(prof)
    wide = int(np.argmax(spread >= 2))
    a, e = int(off[wide]), int(off[wide + 1])
    row = f"pdl_pan_curves: the profile's family {wide} "
    messages = dict(
        families=f"pdl_pan_curves: the profile's genome_off runs from 0 to {int(off[F - 1])}, not from 0 to its {Z} incidences",
        no_family=f"pdl_pan_curves: a profile of {G} genomes, 0 families and {Z} incidences",
        no_genome=f"pdl_pan_curves: a profile of 0 genomes, {F} families and {Z} incidences",
        incidences=f"pdl_pan_curves: the profile's genome_off runs from 0 to {Z}, not from 0 to its {Z + 1} incidences",
        core=f"pdl_pan_curves: the profile says {prof['core'] + 1} core families, its rows hold {prof['core']}",
        descending=row + f"names genome {int(gen[a])} at place 1 of its row (ascending ids below {G})",
        twice=row + f"names genome {int(gen[a])} at place 1 of its row (ascending ids below {G})",
        outside=row + f"names genome {G} at place {e - a - 1} of its row (ascending ids below {G})",
        shifted=f"pdl_pan_curves: the profile's genome_off runs from 1 to {Z}, not from 0 to its {Z} incidences",
        short=f"pdl_pan_curves: the profile's genome_off runs from 0 to {Z - 1}, not from 0 to its {Z} incidences",
        empty_row=row + f"has the row [{a}, {a}) and spread {int(spread[wide])} ({G} genomes)",
        spread=row + f"has the row [{a}, {e}) and spread {int(spread[wide]) + 1} ({G} genomes)",
        null_off="pdl_pan_curves: the profile's genome_off, genomes or spread is NULL",
        null_genomes="pdl_pan_curves: the profile's genome_off, genomes or spread is NULL",
        null_spread="pdl_pan_curves: the profile's genome_off, genomes or spread is NULL")
    for name, changed in both.items():
        o = orders if changed.get("n_genomes") is None else orders[:, :max(1, changed["n_genomes"])].copy()
        rc, msg = _raw_curves(ctx, prof, o, len(orders), **changed)
        assert rc == _lib.PDL_ERR_ARGUMENT, name
        if name in messages:
            assert msg == messages[name], name
    for name, changed in own.items():                 # what the matrices refuse lies in fields the curves do not read
        assert not set(changed) & {"n_genomes", "families", "incidences", "core", "spread", "genome_off", "genomes"}, name
    assert _raw_curves(ctx, prof, orders, len(orders))[0] == _lib.PDL_OK
    rc, msg = _raw_curves(ctx, prof, None, 3)
    assert rc == _lib.PDL_ERR_ARGUMENT and msg == "pdl_pan_curves: NULL pointer"
    big = _one_core_family(_lib.PDL_PAN_MAX_GENOMES + 1)
    rc, msg = _raw_curves(ctx, big, PC.order_set(_lib.PDL_PAN_MAX_GENOMES + 1, 1, 9), 1)
    assert rc == _lib.PDL_ERR_UNSUPPORTED and msg == f"pdl_pan_curves: {_lib.PDL_PAN_MAX_GENOMES + 1} genomes, the kernel's LDS holds an order of at most {_lib.PDL_PAN_MAX_GENOMES}"


# ---- state -------------------------------------------------------------------------------------------------------------------
def test_the_call_leaves_a_scored_context_alone():
    from tests.test_gpu_families import _assert_observables_equal, _assert_same, _native, _observables
    shape, k = CASES["paralogs_6x80x120_k3"]
    gs = make_gene_set(**shape)
    nat = _native(gs, k)
    fam = nat.generate_families()
    before = _observables(nat, gs.genomes)
    prof, want = MC.expected("random, 7 genomes")
    for _ in range(2):
        assert MC.first_difference(nat.genome_matrix(prof), want) is None
    own = PC.profile_numpy(fam["component_of"], gs.genome_of, gs.genomes)                       # the context's own components as a labelling
    assert MC.first_difference(nat.genome_matrix(own), MC.matrices_numpy(fam["component_of"], gs.genome_of, gs.genomes)) is None
    _assert_observables_equal(before, _observables(nat, gs.genomes))
    _assert_same(nat.generate_families(), fam, "families behind the matrices")
    nat.close()


# ---- end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PARALOGS)
def test_command_on_the_paralog_fixtures(name, tmp_path, capsys):
    from pandelos_amd import netclu
    shape, _ = CASES[name]
    faa = tmp_path / "in.faa"
    make_gene_set(**shape).write_faa(faa)
    shared, copies, distance = (tmp_path / n for n in ("s.tsv", "c.tsv", "d.tsv"))
    assert PG.main(["-i", str(faa), "--clus", str(NET / f"{name}.clus"), "--shared", str(shared), "--shared-copies", str(copies),
                    "--distance", str(distance)]) == 0
    assert "bit columns" in capsys.readouterr().out
    names, genome_of = netclu.read_names(faa)
    gen, genome_names = PG.genome_ids(genome_of)
    fam = PG.family_of_from_clus(names, (NET / f"{name}.clus").read_text())
    want = PG.genome_matrix_host(PC.profile_numpy(fam, gen, len(genome_names)))
    assert shared.read_text() == PG.matrix_tsv(want["shared"], genome_names)
    assert copies.read_text() == PG.matrix_tsv(want["shared_copies"], genome_names)
    assert distance.read_text() == PG.matrix_tsv(PG.jaccard_distance(want["shared"]), genome_names)
