"""K-place on the device (pdl_place_query / pdl_placement_of_edges, pandelos_amd/csrc/pdl_place.h).

  * edges: bit for bit and in order what pangenes.bbh_edges gives on the block pdl_query_scores returns, and what pdl_compute_edges(G)
    gives on a second context the same genes were appended to; golden query fixtures and tiny random held-out genomes;
  * placement: every field against the numpy contract (pandelos_amd.place.placement_from_edges) over the base's own edges plus the
    query's, cross-checked against pdl_families_of_edges on the concatenated list;
  * graph shapes no gene set produces, through pdl_placement_of_edges (tests/test_place_cpu.py's SHAPES, the star at full width);
  * state: the base is only read, placements are independent, K-fam on a caller's list in between changes nothing, an append or a
    removal is followed; every refusal returns its code, leaves `out` zeroed and the context usable;
  * the command."""
import ctypes as C
import os

import numpy as np
import pytest

from pandelos_amd import _lib
from pandelos_amd import place as P
from pandelos_amd.pangenes import bbh_edges, net_lines
from tests import helpers as H
from tests.test_gpu_families import _assert_observables_equal, _observables
from tests.test_gpu_query import _native, _random_case
from tests.test_place_cpu import SHAPES, assert_placement, check_expectation, shape
from tests.test_query_golden import CASES, load_case

pytestmark = pytest.mark.gpu
N_SEEDS = int(os.environ.get("PDL_PLACE_SEEDS", "30"))


def _base_edges(nat, genomes):
    parts = [nat.generate_edges_part(g) for g in range(genomes)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _check_case(base, query, k, label):
    """One base, one query: the edges against the host filter and against an appended context, the placement against the contract
    and against K-fam over the concatenated list.  -> the placement."""
    res_b, off_b, gen_b = base
    rq, oq = query
    N, n, G = len(gen_b), len(oq) - 1, int(gen_b.max()) + 1
    nat = _native(k, res_b, off_b, gen_b)
    pl = nat.place_query(rq, oq)
    info = nat.last_place_info
    # edges
    block = nat.query_scores(rq, oq)
    src, dst, score = bbh_edges(block)
    assert np.array_equal(pl["src"], src) and np.array_equal(pl["dst"], dst), f"{label}: edges differ from bbh_edges(query_scores)"
    assert H.raw(pl["score"]).tobytes() == H.raw(score).tobytes(), f"{label}: edge scores differ"
    phase1 = int(np.count_nonzero(np.asarray(pl["dst"]) < N) + np.count_nonzero(np.asarray(pl["src"]) < N))
    assert pl["edges_phase1"] == phase1 and (np.asarray(pl["src"][phase1:]) >= N).all() and (np.asarray(pl["dst"][phase1:]) >= N).all(), label
    assert info["edges"] == len(src) and info["query"]["genome_cost"] == nat.last_query_info["genome_cost"] and info["device_ms"] > 0
    union = _native(k, res_b, off_b, gen_b)
    union.append(rq, oq)
    us, ud, usc = union.generate_edges_part(G)
    assert np.array_equal(us, src) and np.array_equal(ud, dst) and H.raw(usc).tobytes() == H.raw(score).tobytes(), f"{label}: edges differ from the appended context's"
    union.close()
    # placement
    bs, bd = _base_edges(nat, G)
    want = P.placement_from_edges(bs, bd, gen_b, n, src, dst)
    assert_placement(pl, want, label)
    fam = nat.families_of_edges(np.concatenate([bs, src]), np.concatenate([bd, dst]), np.concatenate([gen_b, np.full(n, G, np.uint32)]))
    assert np.array_equal(pl["family_of"], fam["component_of"][N:]) and np.array_equal(pl["is_node"], fam["is_node"][N:]), label
    fam_of = {int(fam["family_genes"][o]): f for f, o in enumerate(fam["family_off"][:-1].tolist())}
    assert [int(fam["collides"][fam_of[int(lab)]]) for lab in pl["group_label"]] == pl["group_collides"].tolist(), label
    again = nat.place_query(rq, oq)                       # (K-fam ran over a caller's list in between)
    assert_placement(again, pl, f"{label} again")
    assert np.array_equal(again["src"], pl["src"]) and np.array_equal(again["dst"], pl["dst"])
    nat.close()
    return pl


@pytest.mark.parametrize("name", CASES)
def test_fixture(name):
    fx, base, query, k, G = load_case(name)
    rq, oq, _ = query.flatten()
    pl = _check_case(base.flatten(), (rq, oq), k, name)
    assert pl["genomes"] == G and pl["n_query"] == len(query.sequences)


def _usable_seeds(count, first=5000):
    """The first `count` seeds that give a usable split (numpy only: decided when the tests are collected, so every case runs)."""
    seeds, seed = [], first
    while len(seeds) < count:
        if _random_case(seed) is not None:
            seeds.append(seed)
        seed += 1
    return seeds


@pytest.mark.parametrize("seed", _usable_seeds(N_SEEDS))
def test_random_small_sets(seed):
    base, query, k = _random_case(seed)
    _check_case(base, query, k, f"seed {seed}")


def _paralog_case():
    from pandelos_amd.synth import make_gene_set
    from tests.test_gpu_query import _split
    gs = make_gene_set(genomes=7, genes_per_genome=60, mean_len=90, sub_rate=0.2, presence=0.8, seed=4242, paralogs=0.4)
    base, query = _split(gs.residues, gs.offsets, gs.genome_of, int(gs.genome_of.max()))
    return base, query, 3


def test_a_set_with_paralogs_has_every_kind_of_group():
    base, query, k = _paralog_case()
    pl = _check_case(base, query, k, "paralogs")
    assert pl["joined"] > 0 and pl["bridging"] > 0 and 0 < pl["colliding"] < pl["groups"] and pl["unplaced"] > 0, {f: pl[f] for f in P.COUNTS}


def test_a_query_identical_to_a_base_genome():
    """Every best score is 1.0: inter_max stays 0, so every row's threshold is 0 and phase 2 keeps every mutual best pair."""
    base, _, k = _paralog_case()
    res_b, off_b, gen_b = base
    off = off_b.astype(np.int64)
    ids = np.nonzero(gen_b == 0)[0]
    oq = np.zeros(len(ids) + 1, np.uint64)
    np.cumsum([off[i + 1] - off[i] for i in ids], out=oq[1:])
    rq = np.concatenate([res_b[off[i]:off[i + 1]] for i in ids]).astype(np.uint8)
    pl = _check_case(base, (rq, oq), k, "identical")
    n1 = pl["edges_phase1"]
    assert n1 > 0 and (H.raw(pl["score"][:n1]) == H.raw(np.float32(1.0))).any()
    assert pl["unplaced"] == 0 and pl["novel"] == 0 and n1 < len(pl["src"])          # (phase-2 edges: paralogs of the copied genome)


# ---- graph shapes through pdl_placement_of_edges ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.open()                        # no preprocess: pdl_placement_of_edges needs none
    yield nat
    nat.close()


@pytest.mark.parametrize("kind", SHAPES)
def test_graph_shapes(kind, ctx):
    bs, bd, genome_of, n, qs, qd, expect = shape(kind, wide=3000)
    base = ctx.families_of_edges(bs, bd, genome_of)
    got = ctx.placement_of_edges(base, genome_of, n, qs, qd)
    assert_placement(got, P.placement_from_edges(bs, bd, genome_of, n, qs, qd), kind)
    check_expectation(got, expect, kind)
    assert "src" not in got and ctx.last_place_info["device_ms"] > 0
    if kind == "star":
        assert got["bridging"] == 1 and len(got["group_base"]) == 3001 and got["group_collides"].tolist() == [1, 0]
    rng = np.random.default_rng(3)                    # order does not matter
    p = rng.permutation(len(qs))
    assert_placement(ctx.placement_of_edges(base, genome_of, n, qd[p], qs[p]), got, f"{kind} shuffled and flipped")


def test_bad_lists_are_refused_on_the_device(ctx):
    bs, bd, genome_of, n, qs, qd, _ = shape("chain")
    base = ctx.families_of_edges(bs, bd, genome_of)
    N = len(genome_of)
    for src, dst in ([N, N + n], [0, 1]), ([N, -1], [0, N]), ([N, 0], [1, 1]), ([1 << 30], [N]):
        with pytest.raises(_lib.PdlError) as e:
            ctx.placement_of_edges(base, genome_of, n, src, dst)
        assert e.value.code == _lib.PDL_ERR_ARGUMENT, e.value
    with pytest.raises(_lib.PdlError) as e:
        ctx.placement_of_edges(base, genome_of, 0, [], [])
    assert e.value.code == _lib.PDL_ERR_ARGUMENT
    # a base whose fields contradict each other: labels reversed; one family listed twice and another left out (node 2 is then in
    # no family and its component_of, here far out of range, would be followed on the device); a genome id past the limit
    fo, fg = base["family_off"], base["family_genes"]
    twice = np.concatenate([fg[fo[0]:fo[1]], fg[fo[0]:fo[1]], fg[fo[2]:]]).astype(np.uint32)
    wild = base["component_of"].copy()
    wild[2] = wild[3] = 1 << 29
    for broken, gen in ((dict(base, component_of=base["component_of"][::-1].copy()), genome_of),
                        (dict(base, family_genes=twice, component_of=wild), genome_of),
                        (dict(base, component_of=wild), genome_of),
                        (base, np.where(np.arange(N) == 3, 0xffffffff, genome_of).astype(np.uint32))):
        with pytest.raises(_lib.PdlError) as e:
            ctx.placement_of_edges(broken, gen, n, qs, qd)
        assert e.value.code == _lib.PDL_ERR_ARGUMENT, e.value
    lib = _lib.load()
    out = _lib.PdlPlacement(groups=7)
    one = np.full(1, N, np.int32)
    assert lib.pdl_placement_of_edges(ctx._ctx, None, genome_of.ctypes.data, n, one.ctypes.data, one.ctypes.data, 1, C.byref(out)) == _lib.PDL_ERR_ARGUMENT
    assert out.groups == 0 and not out.family_of
    got = ctx.placement_of_edges(base, genome_of, n, qs, qd)             # the context is as usable as before
    assert_placement(got, P.placement_from_edges(bs, bd, genome_of, n, qs, qd), "after refusals")


# ---- state -----------------------------------------------------------------------------------------------------------------
def test_the_base_is_only_read_and_placements_are_independent(ctx):
    fx, base, query, k, G = load_case("protein_like_held_out")
    res_b, off_b, gen_b = base.flatten()
    rq, oq, _ = query.flatten()
    nat = _native(k, res_b, off_b, gen_b)
    before = _observables(nat, G)
    fam = nat.generate_families()
    a = nat.place_query(rq, oq)
    other = ctx.families_of_edges([0, 1], [1, 2], np.zeros(3, np.uint32))          # another context's call in between
    assert other["families"] == 1
    mine = nat.families_of_edges([0], [1], np.zeros(2, np.uint32))                 # K-fam over a caller's list on this one
    assert mine["families"] == 1
    half = nat.place_query(rq[:int(oq[2])], oq[:3])                                # another query in between
    assert half["n_query"] == 2
    b = nat.place_query(rq, oq)
    assert_placement(a, b, "two placements")
    assert all(np.array_equal(H.raw(a[f]), H.raw(b[f])) for f in ("src", "dst", "score"))
    _assert_observables_equal(before, _observables(nat, G))
    fam2 = nat.generate_families()
    assert all(np.array_equal(fam[f], fam2[f]) for f in ("component_of", "is_node", "family_off", "family_genes", "collides"))
    nat.close()


def test_families_on_first_use_then_after_an_append_and_a_removal():
    base, query, k = _paralog_case()
    res_b, off_b, gen_b = base
    rq, oq = query
    G = int(gen_b.max()) + 1
    nat = _native(k, res_b, off_b, gen_b)
    first = nat.place_query(rq, oq)                                       # scoring, K-bbh and K-fam run on first use
    assert_placement(first, P.placement_from_edges(*_base_edges(nat, G), gen_b, len(oq) - 1, first["src"], first["dst"]), "first use")
    # the query is appended: a copy of it now finds itself in the base
    nat.append(rq, oq)
    gen_u = np.concatenate([gen_b, np.full(len(oq) - 1, G, np.uint32)])
    after = nat.place_query(rq, oq)
    assert after["sequences"] == len(gen_u) and after["genomes"] == G + 1
    assert_placement(after, P.placement_from_edges(*_base_edges(nat, G + 1), gen_u, len(oq) - 1, after["src"], after["dst"]), "after an append")
    assert np.array_equal(after["src"], bbh_edges(nat.query_scores(rq, oq))[0])
    # ... and leaves again: the first answer is back
    nat.remove([G])
    back = nat.place_query(rq, oq)
    assert_placement(back, first, "after a removal")
    assert all(np.array_equal(H.raw(back[f]), H.raw(first[f])) for f in ("src", "dst", "score"))
    nat.close()


def test_refusals_return_their_code_leave_out_zeroed_and_the_context_usable():
    from pandelos_amd.pangene_native import PangeneNative
    fx, base, query, k, G = load_case("identical_gene")
    res_b, off_b, gen_b = base.flatten()
    rq, oq, _ = query.flatten()
    lib = _lib.load()

    def refused(nat, want, res=rq, off=oq):
        out, info = _lib.PdlPlacement(groups=9, device_ms=1.0), _lib.PdlQueryInfo(records=5)
        res, off = np.ascontiguousarray(res, np.uint8), np.ascontiguousarray(off, np.uint64)
        rc = lib.pdl_place_query(nat._ctx, res.ctypes.data, off.ctypes.data, len(off) - 1, C.byref(out), C.byref(info))
        assert rc == want, (rc, lib.pdl_last_error(nat._ctx))
        assert bytes(out) == bytes(_lib.PdlPlacement()) and bytes(info) == bytes(_lib.PdlQueryInfo())
        return lib.pdl_last_error(nat._ctx).decode()

    nat = PangeneNative.open()
    refused(nat, _lib.PDL_ERR_STATE)                                      # before a preprocess
    nat.preprocess(k, res_b, off_b, gen_b, only_complexity=True)
    refused(nat, _lib.PDL_ERR_STATE)                                      # after only_complexity
    nat.close()
    nat = PangeneNative.open()
    nat.set_genome_shard([0, 1])                                          # a genome shard in force
    nat.preprocess(k, res_b, off_b, gen_b)
    assert "shard" in refused(nat, _lib.PDL_ERR_STATE)
    assert nat.query_scores(rq, oq).scoresCount >= 0                      # ... and the context goes on serving queries
    nat.close()
    nat = PangeneNative.open()
    nat.set_option("low_memory", 1)
    nat.preprocess(k, res_b, off_b, gen_b)
    assert "low_memory" in refused(nat, _lib.PDL_ERR_STATE)
    nat.close()

    nat = _native(k, res_b, off_b, gen_b)
    before = _observables(nat, G)
    msg = refused(nat, _lib.PDL_ERR_UNSUPPORTED, np.frombuffer(b"ACAZZ", np.uint8), np.array([0, 5], np.uint64))
    assert "0x5a" in msg and "'Z'" in msg                                 # the query's own refusal, code and message
    refused(nat, _lib.PDL_ERR_ARGUMENT, rq, np.zeros(1, np.uint64))       # n_query == 0
    refused(nat, _lib.PDL_ERR_ARGUMENT, rq, np.array([0, 5, 3], np.uint64))
    assert lib.pdl_place_query(nat._ctx, rq.ctypes.data, None, 1, C.byref(_lib.PdlPlacement()), None) == _lib.PDL_ERR_ARGUMENT
    assert lib.pdl_place_query(nat._ctx, rq.ctypes.data, oq.ctypes.data, len(oq) - 1, None, None) == _lib.PDL_ERR_ARGUMENT
    assert lib.pdl_place_query(None, rq.ctypes.data, oq.ctypes.data, len(oq) - 1, C.byref(_lib.PdlPlacement()), None) == _lib.PDL_ERR_ARGUMENT
    _assert_observables_equal(before, _observables(nat, G))
    pl = nat.place_query(rq, oq)                                          # still usable after the refusals
    assert_placement(pl, P.placement_from_edges(*_base_edges(nat, G), gen_b, len(oq) - 1, pl["src"], pl["dst"]), "after refusals")
    from pandelos_amd.pangene_idata import PangeneIData
    with pytest.raises(ValueError):
        nat.place_idata(PangeneIData.from_arrays(rq, oq[:3], np.array([0, 1], np.uint32)))
    nat.close()


# ---- the command -----------------------------------------------------------------------------------------------------------
def test_place_command_end_to_end(tmp_path, capsys):
    from pandelos_amd import query as Q
    fx, base, query, k, G = load_case("protein_like_held_out")
    bf, qf = tmp_path / "base.faa", tmp_path / "new.faa"
    bf.write_bytes(fx["base_faa"].tobytes())
    qf.write_bytes(fx["query_faa"].tobytes())
    tsv, net, qnet = tmp_path / "new.tsv", tmp_path / "new.net", tmp_path / "query.net"
    assert P.main(["-i", str(bf), "-k", str(k), "-q", str(qf), "-o", str(tsv), "--net", str(net)]) == 0
    assert Q.main(["-i", str(bf), "-k", str(k), "-q", str(qf), "-o", str(qnet)]) == 0
    assert net.read_bytes() == qnet.read_bytes() and len(net.read_bytes()) > 0
    res_b, off_b, gen_b = base.flatten()
    nat = _native(k, res_b, off_b, gen_b)
    src, dst, score = bbh_edges(nat.query_idata(query))
    want = P.placement_from_edges(*_base_edges(nat, G), gen_b, len(query.sequences), src, dst)
    nat.close()
    names = list(base.sequenceName) + list(query.sequenceName)
    assert tsv.read_text() == P.tsv_text(P.placement_rows(want, names))
    assert net.read_text() == "".join(net_lines(src, dst, score))
    # the label checks of the query command
    two = tmp_path / "two.faa"
    two.write_bytes(fx["query_faa"].tobytes() + b"other\tx1\tp\nACDEFGHIK\n")
    assert P.main(["-i", str(bf), "-k", str(k), "-q", str(two), "-o", str(tmp_path / "no.tsv")]) == 2
    assert "exactly one genome" in capsys.readouterr().err and not (tmp_path / "no.tsv").exists()
