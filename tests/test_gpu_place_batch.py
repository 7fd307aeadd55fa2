"""K-place for a batch on the device (pdl_place_batch / pdl_placement_batch_of_edges, pandelos_amd/csrc/pdl_place_batch.h).

Placement j of a batch is, field for field and byte for byte, what pdl_place_query returns for query j alone on the same context
(only device_ms differs), and what the numpy contract (pandelos_amd.place.placement_from_edges) gives on the base's own edges:
the golden query fixtures as batches, random small sets with an empty stretch in the middle, every kind of group side by side, a
row that leaves the LDS table, chunkings, graph shapes no gene set produces through the callers'-list form, lists refused on the
device, the base only read, the refusals, the command."""
import ctypes as C
import os

import numpy as np
import pytest

from pandelos_amd import _lib
from pandelos_amd import place as P
from tests import helpers as H
from tests.test_gpu_families import _assert_observables_equal, _observables
from tests.test_gpu_place import _base_edges, _paralog_case
from tests.test_gpu_query import _genes, _native, _split
from tests.test_gpu_query_batch import GROUPS, Q1, _random_batch_case
from tests.test_place_cpu import SHAPES, assert_placement, check_expectation, shape
from tests.test_query_golden import load_case

pytestmark = pytest.mark.gpu
N_SEEDS = int(os.environ.get("PDL_PLACE_BATCH_SEEDS", "30"))
EDGES = ("src", "dst", "score")
INFO = ("residues", "kmer_occurrences", "records", "matched_records", "genome_cost")


def assert_same(got, want, label, edges=True):
    """Two placements equal in every count and array (and, bit for bit, in their edges)."""
    assert_placement(got, want, label)
    assert got["edges_phase1"] == want["edges_phase1"], label
    if edges:
        for f in EDGES:
            assert got[f].dtype == want[f].dtype and H.raw(got[f]).tobytes() == H.raw(want[f]).tobytes(), f"{label}: {f} differs"


def check_batch(nat, gen_b, queries, label, base_edges=None):
    """One batch on `nat`: every placement against the single placement of that query on the same context (and its infos) and
    against the contract over the base's own edges.  -> the placements."""
    G = int(np.max(gen_b)) + 1
    pls = nat.place_batch(queries)
    binfo = nat.last_place_batch_info
    assert len(pls) == len(queries) == len(binfo["queries"]) and binfo["chunks"] >= 1 and binfo["device_ms"] > 0, label
    bs, bd = base_edges if base_edges is not None else _base_edges(nat, G)
    for j, (q, pl, pi) in enumerate(zip(queries, pls, binfo["queries"])):
        lab = f"{label}, query {j}"
        single = nat.place_query(*q)
        si = nat.last_place_info
        assert_same(pl, single, lab + " vs the single placement")
        assert pi["edges"] == si["edges"] == len(pl["src"]) and pi["device_ms"] > 0, lab
        assert {f: pi[f] for f in P.COUNTS} == {f: si[f] for f in P.COUNTS}, lab
        assert {f: pi["query"][f] for f in INFO} == {f: si["query"][f] for f in INFO}, lab
        assert_placement(pl, P.placement_from_edges(bs, bd, gen_b, len(q[1]) - 1, pl["src"], pl["dst"]), lab + " vs the contract")
    return pls


# ---- 1. the fixtures as batches ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", GROUPS, ids=lambda g: "+".join(g))
def test_reference_fixtures_as_one_batch(names):
    cases = [load_case(n) for n in names]
    _, base, _, k, G = cases[0]
    res_b, off_b, gen_b = base.flatten()
    nat = _native(k, res_b, off_b, gen_b)
    pls = check_batch(nat, gen_b, [c[2].flatten()[:2] for c in cases], "+".join(names))
    assert all(pl["genomes"] == G and pl["n_query"] == len(c[2].sequences) for pl, c in zip(pls, cases))
    nat.close()


@pytest.mark.parametrize("name", Q1)
def test_fold_cases_coexist_in_one_batch(name):
    """Every q1 base with ALL the q1 queries its alphabet allows in one batch, then the same queries in reverse order."""
    fx, base, own, k, G = load_case(name)
    res_b, off_b, gen_b = base.flatten()
    letters = np.unique(res_b)
    names = [n for n in Q1 if np.isin(load_case(n)[2].flatten()[0], letters).all()]
    assert name in names and len(names) >= 3, names
    queries = [load_case(n)[2].flatten()[:2] for n in names]
    nat = _native(k, res_b, off_b, gen_b)
    check_batch(nat, gen_b, queries + queries[::-1], f"base of {name}")
    nat.close()


# ---- 2. random small sets ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", list(range(7000, 7000 + N_SEEDS)))
def test_random_small_sets_match_the_single_placement_and_the_contract(seed):
    base, queries, k = _random_batch_case(seed)
    # the generator ends with [one gene, genes shorter than k, the first query again]: the query without a k-mer goes into the
    # middle of the batch — an empty stretch of cells, edges and groups between two full ones
    held, (one, short, again) = queries[:-3], queries[-3:]
    queries = [held[0], one, short] + held[1:] + [again]
    nat = _native(k, *base)
    pls = check_batch(nat, base[2], queries, f"seed {seed}")
    assert pls[2]["groups"] == 0 and len(pls[2]["src"]) == 0 and pls[2]["unplaced"] == 3, seed
    assert_same(pls[-1], pls[0], f"seed {seed}: identical queries")       # neither saw the other
    nat.close()


# ---- 3. every kind of group, side by side; 5. chunkings ------------------------------------------------------------------
def _paralog_batch():
    """The paralog set of tests/test_gpu_place.py (7 x 60 genes, k = 3) with three genomes held out as three queries and a fourth
    query identical to base genome 0.  -> (base arrays, queries, k)"""
    from pandelos_amd.synth import make_gene_set
    gs = make_gene_set(genomes=7, genes_per_genome=60, mean_len=90, sub_rate=0.2, presence=0.8, seed=4242, paralogs=0.4)
    res, off, gen = gs.residues, gs.offsets, gs.genome_of.astype(np.int64)
    queries = []
    for held in (6, 5, 4):
        (res, off, gen), q = _split(res, off, gen, held)
        gen = gen.astype(np.int64)
        queries.append(q)
    base = (res, off, gen.astype(np.uint32))
    assert _paralog_case()[1][0].tobytes() == queries[0][0].tobytes()     # (query 0 is that test's query)
    queries.append(_split(res, off, gen, 0)[1])
    return base, queries, 3


def test_every_kind_of_group_side_by_side_under_three_chunkings():
    base, queries, k = _paralog_batch()
    nat = _native(k, *base)
    whole = check_batch(nat, base[2], queries, "paralogs")
    assert nat.last_place_batch_info["chunks"] == 1
    tot = {f: sum(pl[f] for pl in whole) for f in P.COUNTS}
    assert tot["joined"] > 0 and tot["bridging"] > 0 and tot["novel"] + tot["unplaced"] > 0, tot
    assert 0 < tot["colliding"] < tot["groups"], tot                      # colliding and clean groups
    assert whole[3]["unplaced"] == 0 and whole[3]["novel"] == 0           # the copy of base genome 0 finds itself
    assert len({pl["n_query"] for pl in whole}) > 1                       # queries of different sizes

    def run(budget):
        nat.set_option("query_batch_bytes", budget)
        parts = nat.place_batch(queries)
        for j, (x, y) in enumerate(zip(parts, whole)):
            assert_same(x, y, f"budget {budget}, query {j}")
        return nat.last_place_batch_info["chunks"]
    assert run(1) == 4                                                    # chunks of one
    # chunks of two: a chunk takes all the consecutive queries that fit, so the first budget that gives two chunks may cut
    # 2 + 2 or 3 + 1.  A placement's device_ms is an even share of its chunk's, so the shares say which queries shared a chunk:
    # the search goes on until they show 2 + 2 (the four queries weigh nearly the same; between "three fit" and "two fit" lies
    # a budget where the first two fill a chunk and the last two the next)
    seen, cut = {}, None
    for budget in range(200_000, 4_000_000, 20_000):
        seen[budget] = run(budget)
        ms = [q["device_ms"] for q in nat.last_place_batch_info["queries"]]
        if seen[budget] == 2 and ms[0] == ms[1] and ms[2] == ms[3] and ms[1] != ms[2]:
            cut = budget
            break
        if seen[budget] < 2:
            break
    assert cut is not None, seen
    assert run(1 << 30) == 1
    nat.close()


# ---- 4. a row that leaves the LDS table ----------------------------------------------------------------------------------
def test_a_wide_row_among_queries_of_other_sizes():
    fx, base, query, k, G = load_case("wide_row_9000_columns")
    res_b, off_b, gen_b = base.flatten()
    wide = query.flatten()[:2]
    nat = _native(k, res_b, off_b, gen_b)
    queries = [_genes(b"AAAA", b"CDEFAAA", b"AAAD", b"KLAAAC"), wide, _genes(b"ACDEF"), _genes(b"AAAC", b"ACDEF", b"AAAK", b"EFG", b"AAAAA", b"HIKAAA")]
    block = nat.query_scores(*wide)
    assert int((np.asarray(block.row) == np.asarray(block.row)[0]).sum()) > 8192      # (its cells come from the HBM-table join)
    check_batch(nat, gen_b, queries, "wide row")
    nat.close()


# ---- 6. graph shapes through pdl_placement_batch_of_edges ----------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.open()                        # no preprocess: the callers'-list form needs none
    yield nat
    nat.close()


@pytest.fixture(scope="module")
def shapes_union():
    """One base: the disjoint union of the bases of SHAPES, ids shifted; per shape its query list in ITS union ids of the big base.
    -> (base_src, base_dst, genome_of, [(kind, n, src, dst, expect)])"""
    parts = [shape(kind, wide=3000) for kind in SHAPES]
    N = sum(len(p[2]) for p in parts)
    bs, bd, gen, lists, at = [], [], [], [], 0
    for kind, (s, d, genome_of, n, qs, qd, expect) in zip(SHAPES, parts):
        Nk = len(genome_of)
        bs.append(s + at); bd.append(d + at); gen.append(genome_of)
        move = lambda x: np.where(x < Nk, x + at, x - Nk + N)             # base ids shift, query ids start at the big base's N
        lists.append((kind, n, move(qs), move(qd), expect))
        at += Nk
    return np.concatenate(bs), np.concatenate(bd), np.concatenate(gen).astype(np.uint32), lists


def test_graph_shapes_in_one_batch(ctx, shapes_union):
    bs, bd, genome_of, lists = shapes_union
    base = ctx.families_of_edges(bs, bd, genome_of)
    both = lists + lists[::-1]                        # every shape twice: two queries of one batch touch the same base components
    want = [P.placement_from_edges(bs, bd, genome_of, n, qs, qd) for _, n, qs, qd, _ in lists]
    want = want + want[::-1]
    got = ctx.placement_batch_of_edges(base, genome_of, [n for _, n, _, _, _ in both], [(qs, qd) for _, _, qs, qd, _ in both])
    assert len(got) == 2 * len(SHAPES)
    for (kind, n, qs, qd, expect), pl, w in zip(both, got, want):
        assert_placement(pl, w, kind)
        check_expectation(pl, expect, kind)
        assert "src" not in pl
        assert_placement(pl, ctx.placement_of_edges(base, genome_of, n, qs, qd), f"{kind} vs the single list")
    star = got[SHAPES.index("star")]
    assert star["bridging"] == 1 and len(star["group_base"]) == 3001
    rng = np.random.default_rng(3)                    # order and direction inside a list do not matter
    mixed = []
    for _, _, qs, qd, _ in both:
        p = rng.permutation(len(qs))
        mixed.append((qd[p], qs[p]))
    for (kind, *_), pl, w in zip(both, ctx.placement_batch_of_edges(base, genome_of, [n for _, n, _, _, _ in both], mixed), got):
        assert_placement(pl, w, f"{kind} shuffled and flipped")


# ---- 7. bad lists refused on the device ----------------------------------------------------------------------------------
def test_bad_lists_are_refused_on_the_device(ctx):
    bs, bd, genome_of, _, _, _, _ = shape("chain")
    base = ctx.families_of_edges(bs, bd, genome_of)
    N = len(genome_of)
    n_query = [2, 3, 5]                               # three queries of different sizes; the middle one is broken in turn
    good = [([N, N + 1], [0, N]), ([N, 1, N + 2], [N + 1, N + 2, 2]), ([N + 4, N + 3], [3, N + 4])]
    want = [P.placement_from_edges(bs, bd, genome_of, n, s, d) for n, (s, d) in zip(n_query, good)]
    lib = _lib.load()
    fam, g, keep = ctx._base_families(base, genome_of)
    nq = np.asarray(n_query, np.uint32)
    for bad in (([N, N + 3], [0, N]),                 # an id N + n_1 that the largest query would accept
                ([N, -1], [0, N]),                    # a negative id
                ([N, 0], [1, 1])):                    # a base-base edge
        lists = [good[0], bad, good[2]]
        with pytest.raises(_lib.PdlError) as e:
            ctx.placement_batch_of_edges(base, genome_of, n_query, lists)
        assert e.value.code == _lib.PDL_ERR_ARGUMENT and "query 1" in str(e.value), e.value
        s, d, begin = ctx.pack_edge_lists(lists)
        out = (_lib.PdlPlacement * 3)()
        for o in out:
            o.groups, o.device_ms = 7, 1.0            # stale values: a refusal must leave `out` zeroed
        rc = lib.pdl_placement_batch_of_edges(ctx._ctx, C.byref(fam), g.ctypes.data, 3, nq.ctypes.data, begin.ctypes.data, s.ctypes.data, d.ctypes.data, out)
        assert rc == _lib.PDL_ERR_ARGUMENT and all(bytes(o) == bytes(_lib.PdlPlacement()) for o in out)
        for pl, w in zip(ctx.placement_batch_of_edges(base, genome_of, n_query, good), want):      # the context is as usable as before
            assert_placement(pl, w, "after a refused list")
    # the first failing query is named when two fail
    with pytest.raises(_lib.PdlError) as e:
        ctx.placement_batch_of_edges(base, genome_of, n_query, [good[0], ([N, 0], [1, 1]), ([N + 5], [0])])
    assert "query 1" in str(e.value)
    # the arguments
    s, d, begin = ctx.pack_edge_lists(good)
    out = (_lib.PdlPlacement * 3)()
    call = lambda fam_p=C.byref(fam), q=3, nq_=nq, begin_=begin, s_=s, out_=out: lib.pdl_placement_batch_of_edges(
        ctx._ctx, fam_p, g.ctypes.data, q, None if nq_ is None else nq_.ctypes.data, None if begin_ is None else begin_.ctypes.data,
        None if s_ is None else s_.ctypes.data, d.ctypes.data, out_)
    A = _lib.PDL_ERR_ARGUMENT
    assert call(fam_p=None) == A and call(q=0) == A and call(nq_=None) == A and call(begin_=None) == A and call(s_=None) == A and call(out_=None) == A
    assert call(nq_=np.array([2, 0, 5], np.uint32)) == A
    down = begin.copy(); down[1], down[2] = begin[2], begin[1]
    assert call(begin_=down) == A
    with pytest.raises(_lib.PdlError) as e:
        ctx.placement_batch_of_edges(dict(base, component_of=base["component_of"][::-1].copy()), genome_of, n_query, good)
    assert e.value.code == A
    assert call() == _lib.PDL_OK
    for o in out:
        lib.pdl_free_placement(C.byref(o))
    del keep


# ---- 8. the base is only read; work buffers are shared safely -----------------------------------------------------------
def test_the_base_is_only_read_and_the_other_entry_points_answer_as_before():
    fx, base, query, k, G = load_case("protein_like_held_out")
    res_b, off_b, gen_b = base.flatten()
    q = query.flatten()[:2]
    half = (q[0][: int(q[1][len(q[1]) // 2])].copy(), q[1][: len(q[1]) // 2 + 1].copy())
    queries = [half, q, _genes(b"ACDEFGHIK"), half]
    nat = _native(k, res_b, off_b, gen_b)
    before = _observables(nat, G)
    fam = nat.generate_families()
    single = nat.place_query(*q)
    blocks = [b.as_dict() for b in nat.query_batch(queries)]
    scores = nat.query_scores(*q).as_dict()
    pls = check_batch(nat, gen_b, queries, "held out")
    assert_same(pls[3], pls[0], "identical queries")
    _assert_observables_equal(before, _observables(nat, G))
    fam2 = nat.generate_families()
    assert all(np.array_equal(fam[f], fam2[f]) for f in ("component_of", "is_node", "family_off", "family_genes", "collides"))
    assert_same(nat.place_query(*q), single, "place_query after the batch")
    for j, (x, y) in enumerate(zip(nat.query_batch(queries), blocks)):
        H.assert_scores_equal(x.as_dict(), y, f"query_batch after the batch, query {j}")
    H.assert_scores_equal(nat.query_scores(*q).as_dict(), scores, "query_scores after the batch")
    # after an append the batch answers for the union
    nat.append(*half)
    gen_u = np.concatenate([gen_b, np.full(len(half[1]) - 1, G, np.uint32)])
    after = check_batch(nat, gen_u, [q, half], "after an append")
    assert after[0]["sequences"] == len(gen_u) and after[0]["genomes"] == G + 1
    nat.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_return_their_code_leave_out_zeroed_and_the_context_usable():
    from pandelos_amd.pangene_native import PangeneNative
    fx, base, query, k, G = load_case("identical_gene")
    res_b, off_b, gen_b = base.flatten()
    rq, oq, _ = query.flatten()
    good = (rq, oq)
    lib = _lib.load()
    res, off, begin = PangeneNative.pack_queries([good, good, good, good])
    n = len(off) - 1

    def raw(nat, res=res, off=off, begin=begin, n=n, q=4, out=True, null_res=False):
        pls = (_lib.PdlPlacement * 4)()
        for p in pls:                                                     # stale values: a refusal must leave `out` zeroed
            p.groups, p.device_ms = 77, 8.0
        infos = (_lib.PdlQueryInfo * 4)()
        for i in infos:
            i.records = 5
        binfo = _lib.PdlPlaceBatchInfo(queries=9, chunks=9)
        rc = lib.pdl_place_batch(nat._ctx, None if null_res else res.ctypes.data, None if off is None else off.ctypes.data,
                                 None if begin is None else begin.ctypes.data, n, q, pls if out else None, infos, C.byref(binfo))
        if rc != _lib.PDL_OK:
            assert bytes(binfo) == bytes(_lib.PdlPlaceBatchInfo())
            if out:
                assert all(bytes(p) == bytes(_lib.PdlPlacement()) for p in pls[:q]), "out is not zeroed after a refusal"
                assert all(bytes(i) == bytes(_lib.PdlQueryInfo()) for i in infos[:q])
        else:
            for p in pls:
                lib.pdl_free_placement(C.byref(p))
        return rc, lib.pdl_last_error(nat._ctx).decode()

    # every state pdl_place_query refuses
    S, A, U = _lib.PDL_ERR_STATE, _lib.PDL_ERR_ARGUMENT, _lib.PDL_ERR_UNSUPPORTED
    nat = PangeneNative.open()
    assert raw(nat)[0] == S                                               # before a preprocess
    nat.preprocess(k, res_b, off_b, gen_b, only_complexity=True)
    assert raw(nat)[0] == S                                               # after only_complexity
    nat.close()
    nat = PangeneNative.open()
    nat.set_genome_shard([0, 1])                                          # a genome shard in force
    nat.preprocess(k, res_b, off_b, gen_b)
    rc, msg = raw(nat)
    assert rc == S and "shard" in msg and "pdl_placement_batch_of_edges" in msg
    assert len(nat.query_batch([good])) == 1                              # ... and the context goes on serving queries
    nat.close()
    nat = PangeneNative.open()
    nat.set_option("low_memory", 1)
    nat.preprocess(k, res_b, off_b, gen_b)
    rc, msg = raw(nat)
    assert rc == S and "low_memory" in msg
    nat.close()

    nat = _native(k, res_b, off_b, gen_b)
    before = _observables(nat, G)
    want = nat.place_query(*good)
    assert raw(nat)[0] == _lib.PDL_OK
    assert raw(nat, q=0)[0] == A
    assert raw(nat, n=0, begin=np.zeros(5, np.uint32))[0] == A
    assert raw(nat, off=None)[0] == A and raw(nat, begin=None)[0] == A and raw(nat, out=False)[0] == A and raw(nat, null_res=True)[0] == A
    bad_off = off.copy(); bad_off[2] = bad_off[1] - 1
    assert raw(nat, off=bad_off)[0] == A
    u32 = lambda *v: np.array(v, np.uint32)
    per = int(begin[1])
    for bad_begin in (u32(1, per, 2 * per, 3 * per, n),                   # does not start at 0
                      u32(0, per, 2 * per, 3 * per, n - 1),               # does not end at n
                      u32(0, per, 2 * per, 3 * per, n + 1),               # ends past n
                      u32(0, per, per, 3 * per, n),                       # a query without genes
                      u32(0, 2 * per, per, 3 * per, n)):                  # decreasing
        rc, msg = raw(nat, begin=bad_begin)
        assert rc == A and "pdl_place_batch" in msg, msg
        assert_same(nat.place_batch([good])[0], want, "a valid call after a refusal")
    # a byte the base lacks in query 2 of 4 (and a smaller one in query 3): the first such query — also under chunks of one,
    # when the placements of the earlier chunks had been made
    z = (np.frombuffer(b"ACAZZX", np.uint8).copy(), np.array([0, 6], np.uint64))
    z3 = (np.frombuffer(b"ACAB", np.uint8).copy(), np.array([0, 4], np.uint64))
    r4, o4, b4 = PangeneNative.pack_queries([good, good, z, z3])
    for budget in (1 << 30, 1):
        nat.set_option("query_batch_bytes", budget)
        rc, msg = raw(nat, res=r4, off=o4, begin=b4, n=len(o4) - 1)
        assert rc == U and "query 2" in msg and "0x58" in msg and "'X'" in msg, msg
        with pytest.raises(_lib.PdlError) as e:
            nat.place_batch([good, good, z, z3])
        assert e.value.code == U and "query 2" in str(e.value)
        pls = nat.place_batch([good, good])
        assert nat.last_place_batch_info["chunks"] == (1 if budget > 1 else 2)
        assert_same(pls[1], want, f"budget {budget}: a valid call after the refusal")
    nat.set_option("query_batch_bytes", 1 << 30)
    long_gene = (np.resize(rq, (1 << 20) + k + 3).astype(np.uint8), np.array([0, (1 << 20) + k + 3], np.uint64))
    with pytest.raises(_lib.PdlError) as e:
        nat.place_batch([good, long_gene])
    assert e.value.code == U and "2^20" in str(e.value) and "query 1" in str(e.value)
    assert lib.pdl_place_batch(None, res.ctypes.data, off.ctypes.data, begin.ctypes.data, n, 4, (_lib.PdlPlacement * 4)(), None, None) == A
    _assert_observables_equal(before, _observables(nat, G))
    assert_same(nat.place_batch([good])[0], want, "after the refusals")
    from pandelos_amd.pangene_idata import PangeneIData
    with pytest.raises(ValueError):
        nat.place_batch_idata([PangeneIData.from_arrays(rq, oq[:3], np.array([0, 1], np.uint32))])
    nat.close()


# ---- 10. the command -----------------------------------------------------------------------------------------------------
def test_place_batch_command_end_to_end(tmp_path):
    from pandelos_amd import place_batch as PB
    fx, base, query, k, G = load_case("protein_like_held_out")
    bf = tmp_path / "base.faa"
    bf.write_bytes(fx["base_faa"].tobytes())
    recs = list(zip(query.sequenceName, query.sequenceDescription, query.sequences))
    half = len(recs) // 2

    def faa(label, part):
        return b"".join(f"{label}\t{n}\t{d}\n".encode("latin-1") + s + b"\n" for n, d, s in part)
    label = query.genomeNames[0]
    singles = {label: faa(label, recs), "left_half": faa("left_half", recs[:half]), "right-half.2": faa("right-half.2", recs[half:])}
    f1, f2 = tmp_path / "q1.faa", tmp_path / "q2.faa"
    # genomes interleaved inside a file: first-seen order, genes in file order
    f1.write_bytes(b"".join(faa(label, [a]) + faa("left_half", [b]) for a, b in zip(recs[:half], recs[:half])) + faa(label, recs[half:]))
    f2.write_bytes(singles["right-half.2"])
    out = tmp_path / "out"
    assert PB.main(["-i", str(bf), "-k", str(k), "-q", str(f1), "-q", str(f2), "--out-dir", str(out), "--net"]) == 0
    assert sorted(p.name for p in out.iterdir()) == sorted([f"{x}.net" for x in singles] + [f"{x}.tsv" for x in singles])
    for name, data in singles.items():
        qf, tsv, net = tmp_path / f"single_{name}.faa", tmp_path / f"single_{name}.tsv", tmp_path / f"single_{name}.net"
        qf.write_bytes(data)
        assert P.main(["-i", str(bf), "-k", str(k), "-q", str(qf), "-o", str(tsv), "--net", str(net)]) == 0
        assert (out / f"{name}.tsv").read_bytes() == tsv.read_bytes() and len(tsv.read_bytes()) > 0, name
        assert (out / f"{name}.net").read_bytes() == net.read_bytes(), name
    assert (out / f"{label}.net").stat().st_size > 0
    only = tmp_path / "only_tsv"
    assert PB.main(["-i", str(bf), "-k", str(k), "-q", str(f2), "--out-dir", str(only)]) == 0
    assert [p.name for p in only.iterdir()] == ["right-half.2.tsv"]
