"""The pan-genome profile on the device (pdl_family_profile, pdl_pan_curves; pandelos_amd/csrc/pdl_profile.h): every count and
every array element equals the references of tests/profile_cases.py (test_profile_cpu.py holds those against each other), every
refusal has its code, and neither call touches the context it runs on."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from pandelos_amd import _lib
from pandelos_amd import pangenome as PG
from pandelos_amd.synth import make_gene_set
from tests import helpers as H
from tests import profile_cases as PC
from tests.test_host_net import CASES

pytestmark = pytest.mark.gpu
NET, QUALITY = H.GOLDEN / "net", H.GOLDEN / "quality"
PARALOGS = ("paralogs_6x80x120_k3", "paralogs_10x60x90_k3_div20")


@pytest.fixture(scope="module")
def ctx():
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.open()                        # no preprocess: neither call needs one
    yield nat
    nat.close()


def _poison(ctx):
    """Leaves the context's work buffers full of another set's keys, runs, histograms, bits and curves: a kernel that trusted a
    buffer it should have cleared or written shows in the call behind this one."""
    n, G = 9001, 130
    fam, gen = (np.arange(n, dtype=np.uint32) * 13) % 4500, (np.arange(n, dtype=np.uint32) * 29) % G
    prof = ctx.family_profile(fam, gen, G)
    ctx.pan_curves(prof, np.tile(np.arange(G, dtype=np.uint32)[::-1], (3, 1)))


@pytest.mark.parametrize("name", list(PC.profile_cases()))
def test_profile_cases(name, ctx):
    f, g, G = PC.profile_cases()[name]
    _poison(ctx)
    got = ctx.family_profile(f, g, G)
    assert PC.first_difference(got, PC.expected_profile(name)) is None, name
    info = ctx.last_profile_info
    assert info["families"] == got["families"] and info["incidences"] == got["incidences"] and info["device_ms"] > 0
    assert got["core"] + got["unique"] + got["accessory"] == got["families"] + (got["core"] if G == 1 else 0)
    assert got["spread_by_genome"].shape == (G + 1, G) and int(got["genome_genes"].sum()) == len(f)


def test_profile_twice_alike_and_on_two_contexts(ctx):
    from pandelos_amd.pangene_native import PangeneNative
    f, g, G = PC.profile_cases()["random, seed 1"]
    other = PangeneNative.open()
    a, b, c = ctx.family_profile(f, g, G), other.family_profile(f, g, G), ctx.family_profile(f, g, G)
    other.close()
    assert PC.first_difference(a, b) is None and PC.first_difference(a, c) is None


@pytest.mark.parametrize("name", list(PC.curve_cases()))
def test_curve_cases(name, ctx):
    (f, g, G), orders = PC.curve_cases()[name]
    want_profile, want = PC.expected_curves(name)
    _poison(ctx)
    prof = ctx.family_profile(f, g, G)
    assert PC.first_difference(prof, want_profile) is None
    got = ctx.pan_curves(prof, orders)
    assert PC.first_curve_difference(got, want) is None, name
    assert (got["pan"][:, -1] == prof["families"]).all() and (got["core"][:, -1] == prof["core"]).all()
    assert (got["pan"][:, 0] == got["core"][:, 0]).all()
    info = ctx.last_curves_info
    assert info == {"families": prof["families"], "incidences": prof["incidences"], "orders": len(orders), "device_ms": info["device_ms"]}
    assert info["device_ms"] > 0
    assert PC.first_curve_difference(ctx.pan_curves(want_profile, orders), want) is None       # a profile made on the host is as good


def test_curves_at_the_bound_of_the_genome_count(ctx):
    """PDL_PAN_MAX_GENOMES genomes are taken (the order, its inverse and both histograms fill the workgroup's LDS); one more is
    PDL_ERR_UNSUPPORTED with the bound in the message."""
    G = _lib.PDL_PAN_MAX_GENOMES
    assert G >= 4096
    f, g, _ = PC.spread_labelling(G, 40, seed=8)
    prof, orders = PC.profile_numpy(f, g, G), PC.order_set(G, 3, 8)
    got = ctx.pan_curves(prof, orders)
    assert PC.first_curve_difference(got, PG.pan_curves_host(prof, orders)) is None
    assert prof["core"] >= 10 and (got["core"][:, -1] == prof["core"]).all()
    f, g, _ = PC.spread_labelling(G + 1, 8, seed=9)
    with pytest.raises(_lib.PdlError) as e:
        ctx.pan_curves(PC.profile_numpy(f, g, G + 1), PC.order_set(G + 1, 2, 9))
    assert e.value.code == _lib.PDL_ERR_UNSUPPORTED and str(G) in str(e.value)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _raw_profile(ctx, fam, gen, n, G, out=True, handle=True):
    p = _lib.PdlProfile()
    rc = ctx._lib.pdl_family_profile(ctx._ctx if handle else None, None if fam is None else fam.ctypes.data, None if gen is None else gen.ctypes.data,
                                     n, G, C.byref(p) if out else None)
    assert rc == _lib.PDL_OK or (not p.label and not p.genomes and not p.spread_by_genome and p.families == 0)
    ctx._lib.pdl_free_profile(C.byref(p))
    return rc


def test_profile_refusals_and_the_next_call_is_right(ctx):
    f, g, G = PC.profile_cases()["a genome without a gene"]
    want = PC.expected_profile("a genome without a gene")
    n = len(f)
    assert _raw_profile(ctx, f, g, n, G) == _lib.PDL_OK
    for args in ((None, g, n, G), (f, None, n, G), (f, g, 0, G), (f, g, n, 0)):
        assert _raw_profile(ctx, *args) == _lib.PDL_ERR_ARGUMENT, args
    assert _raw_profile(ctx, f, g, n, G, out=False) == _lib.PDL_ERR_ARGUMENT
    assert _raw_profile(ctx, f, g, n, G, handle=False) == _lib.PDL_ERR_ARGUMENT
    for fam, gen, count in ((np.array([0, 5, 2, 3, 3], np.uint32), g, 1),                       # a label = N
                            (f, np.array([0, 4, 3, 0, 7], np.uint32), 2),                       # genome ids = G and above
                            (np.array([0, 0xffffffff, 2, 3, 3], np.uint32), np.array([4, 3, 3, 0, 0], np.uint32), 2)):
        with pytest.raises(_lib.PdlError) as e:
            ctx.family_profile(fam, gen, G)
        assert e.value.code == _lib.PDL_ERR_ARGUMENT and f"{count} genes" in str(e.value), str(e.value)
        assert PC.first_difference(ctx.family_profile(f, g, G), want) is None
    with pytest.raises(_lib.PdlError) as e:
        ctx.family_profile(f, g, 8193)
    assert e.value.code == _lib.PDL_ERR_UNSUPPORTED and "8192" in str(e.value)
    with pytest.raises(ValueError):
        ctx.family_profile(f, g[:-1], G)


def _raw_curves(ctx, prof, orders, n_orders, out=True, handle=True, **changed):
    keep = {n: np.ascontiguousarray(changed.get(n, prof[n]), dtype=np.uint32) for n in ("spread", "genome_off", "genomes") if changed.get(n, 0) is not None}
    p = _lib.PdlProfile(**{n: int(changed.get(n, prof[n])) for n in ("n_genomes", "families", "incidences", "core")})
    for n, a in keep.items():                         # (an array that is left out stays a NULL pointer)
        setattr(p, n, a.ctypes.data_as(_lib._pu32))
    cv = _lib.PdlCurves()
    rc = ctx._lib.pdl_pan_curves(ctx._ctx if handle else None, C.byref(p) if prof is not None and changed.get("profile", 0) is not None else None,
                                 None if orders is None else orders.ctypes.data, n_orders, C.byref(cv) if out else None)
    assert rc == _lib.PDL_OK or (not cv.pan and not cv.core and cv.n_orders == 0)
    ctx._lib.pdl_free_curves(C.byref(cv))
    return rc, ctx._lib.pdl_last_error(ctx._ctx).decode()


def test_curve_refusals_and_the_next_call_is_right(ctx):
    (f, g, G), orders = PC.curve_cases()["257 orders"]
    prof, want = PC.expected_curves("257 orders")
    n = len(orders)
    assert _raw_curves(ctx, prof, orders, n)[0] == _lib.PDL_OK
    assert _raw_curves(ctx, prof, None, n)[0] == _lib.PDL_ERR_ARGUMENT
    assert _raw_curves(ctx, prof, orders, 0)[0] == _lib.PDL_ERR_ARGUMENT
    assert _raw_curves(ctx, prof, orders, n, profile=None)[0] == _lib.PDL_ERR_ARGUMENT
    assert _raw_curves(ctx, prof, orders, n, out=False)[0] == _lib.PDL_ERR_ARGUMENT
    assert _raw_curves(ctx, prof, orders, n, handle=False)[0] == _lib.PDL_ERR_ARGUMENT
    # a profile whose fields contradict each other
    off, gen, spread = prof["genome_off"], prof["genomes"], prof["spread"]
    wide = int(np.argmax(spread >= 2))
    swapped = gen.copy(); swapped[off[wide]:off[wide] + 2] = swapped[off[wide]:off[wide] + 2][::-1]
    twice = gen.copy(); twice[off[wide] + 1] = twice[off[wide]]
    outside = gen.copy(); outside[off[wide + 1] - 1] = G
    shifted = off.copy(); shifted[0] = 1
    short = off.copy(); short[-1] -= 1
    empty = off.copy(); empty[wide + 1] = empty[wide]
    other_spread = spread.copy(); other_spread[wide] += 1
    contradictions = dict(families=dict(families=prof["families"] - 1), no_family=dict(families=0), no_genome=dict(n_genomes=0),
                          incidences=dict(incidences=prof["incidences"] + 1), core=dict(core=prof["core"] + 1), fewer_genomes=dict(n_genomes=G - 1),
                          descending=dict(genomes=swapped), twice=dict(genomes=twice), outside=dict(genomes=outside), shifted=dict(genome_off=shifted),
                          short=dict(genome_off=short), empty_row=dict(genome_off=empty), spread=dict(spread=other_spread),
                          null_off=dict(genome_off=None), null_genomes=dict(genomes=None), null_spread=dict(spread=None))
    for name, changed in contradictions.items():
        o = orders if changed.get("n_genomes") is None else orders[:, :max(1, changed["n_genomes"])].copy()
        assert _raw_curves(ctx, prof, o, n, **changed)[0] == _lib.PDL_ERR_ARGUMENT, name
        assert PC.first_curve_difference(ctx.pan_curves(prof, orders), want) is None, f"behind {name}"
    # an order that is no permutation: the message names the first one
    for where, what in (((3, 5), G), ((200, 0), 0xffffffff), ((5, 2), None), ((256, G - 1), None), ((0, 0), None)):
        bad = orders.copy()
        bad[where] = bad[where[0], (where[1] + 1) % G] if what is None else what               # named twice, or too large
        bad[230, 4] = bad[230, 5] if where[0] < 230 else bad[230, 4]                           # a later order fails as well
        rc, msg = _raw_curves(ctx, prof, bad, n)
        assert rc == _lib.PDL_ERR_ARGUMENT and f"order {where[0]} is the first" in msg, msg
        assert PC.first_curve_difference(ctx.pan_curves(prof, orders), want) is None
    with pytest.raises(ValueError):
        ctx.pan_curves(prof, orders[:, :-1])


# ---- state -------------------------------------------------------------------------------------------------------------------
def test_both_calls_leave_a_scored_context_alone():
    from tests.test_gpu_families import _assert_observables_equal, _assert_same, _native, _observables
    shape, k = CASES["paralogs_6x80x120_k3"]
    gs = make_gene_set(**shape)
    nat = _native(gs, k)
    fam = nat.generate_families()
    before = _observables(nat, gs.genomes)
    (f, g, G), orders = PC.curve_cases()["random labelling"]
    want_profile, want = PC.expected_curves("random labelling")
    for _ in range(2):
        prof = nat.family_profile(f, g, G)
        assert PC.first_difference(prof, want_profile) is None
        assert PC.first_curve_difference(nat.pan_curves(prof, orders), want) is None
    own = nat.family_profile(fam["component_of"], gs.genome_of, gs.genomes)                    # the context's own components as a labelling
    assert PC.first_difference(own, PC.profile_numpy(fam["component_of"], gs.genome_of, gs.genomes)) is None
    _assert_observables_equal(before, _observables(nat, gs.genomes))
    _assert_same(nat.generate_families(), fam, "families behind the profile")
    nat.close()


# ---- end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PARALOGS)
def test_command_on_the_paralog_fixtures(name, tmp_path, capsys):
    shape, k = CASES[name]
    faa = tmp_path / "in.faa"
    make_gene_set(**shape).write_faa(faa)
    want = (QUALITY / f"{name}.txt").read_text()
    q1, q2, clus, matrix, curves = (tmp_path / n for n in ("q1.txt", "q2.txt", "out.clus", "m.tsv", "c.tsv"))
    assert PG.main(["-i", str(faa), "--clus", str(NET / f"{name}.clus"), "--quality", str(q1), "--matrix", str(matrix),
                    "--curves", str(curves), "--orders", "50", "--seed", "3"]) == 0
    assert q1.read_text() == want
    assert "50 orders" in capsys.readouterr().out
    rows = curves.read_text().splitlines()
    assert len(rows) == shape["genomes"] + 1 and len(matrix.read_text().splitlines()) == len((NET / f"{name}.clus").read_text().splitlines()) + 1
    last = rows[-1].split("\t")
    assert last[0] == str(shape["genomes"]) and last[2] == last[3] == str(len(matrix.read_text().splitlines()) - 1)       # pan ends at F in every order
    assert PG.main(["-i", str(faa), "-k", str(k), "-o", str(clus), "--quality", str(q2)]) == 0
    assert clus.read_text() == (NET / f"{name}.clus").read_text() and q2.read_text() == want
    with pytest.raises(SystemExit):
        PG.main(["-i", str(faa)])
