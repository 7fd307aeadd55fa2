"""The query's join at its table, chunk and HBM-table limits (pdl_query.h: q_walk_row, q_row_lds, q_row_hbm, k_q_join, k_q_join_hbm;
pdl_query_batch.h: k_qb_join, k_qb_join_hbm), on the planted rows of tests/query_join_sets.py.

Every case runs through pdl_query_scores — the block bit for bit and in emission order against the CPU oracle's block of genome G of
the union, the genome cost against the oracle's, pdl_get_query_join_info against the plan — a second time on the tables the first
left, and as the middle one of a batch beside two small unrelated queries.  The table sequence and the 33-row case run again with
every query a chunk of its own; four cases go through pdl_place_query and pdl_place_batch, the qextra fold among them.  The
union's fold inside a group of 3900 and of 3000 members, sums near 2^20 and rows that genes of their own query carry over the limit
are the RawCases of the sets module.  After every case the context takes
another base and must still give the wide_row_9000_columns fixture and a tiny query: a table left dirty shows there, and in the
second run of the case itself.

tests/test_query_join_sets_cpu.py holds every case against its plan without a device."""
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import query_join_sets as S
from tests.test_gpu_order_subwave import SETTINGS
from tests.test_query_golden import assert_block, load_case

pytestmark = pytest.mark.gpu
PLACED = ("A-single-%d" % S.MUST_LEAVE, "E-17-rows", "G-qextra-wide", "D-leaves-in-chunk-1")


def _case(name):
    return S.raw_case(name) if name[0] in "GHI" else S.case(name)


@functools.lru_cache(maxsize=None)
def _want(name, q):
    """(the oracle's block of genome G of base + query q, its genome cost); made once, never changed"""
    from oracle import binding as ob
    res, off, gen, G = _case(name).union(q)
    ora = ob.Oracle(res, off, gen, S.K)
    out = ora.scores(G), int(ora.genome_cost(G))
    ora.close()
    return out


@functools.lru_cache(maxsize=None)
def _want_small(name, j):
    """the same for the j-th of the two small queries of a batch, over the case's base"""
    from oracle import binding as ob
    c = _case(name)
    if isinstance(c, S.RawCase):                              # (a filler of its own, twice or once)
        small = S.RawCase(c.name + "-small", c.base_genes, [S.JE.filler(26001 + j, 15)] * (2 - j), None, 0)
        res, off, gen, G = small.union()
        ora = ob.Oracle(res, off, gen, S.K)
        out = ora.scores(G), small.query()
        ora.close()
        return out
    small = S.Case(c.name + "-small", c.nw, c.n_col, c.holders, [S.small_queries(c.nw)[j]], padding=c.padding, extra_seps=tuple(c.seps))
    assert small.N == c.N and np.array_equal(small.base[0], c.base[0])
    res, off, gen, G = small.union(0)
    ora = ob.Oracle(res, off, gen, S.K)
    out = ora.scores(G), small.query(0)
    ora.close()
    return out


@functools.lru_cache(maxsize=None)
def _want_probe(name, n):
    """the oracle's block for the case's probe query of n genes: a cell in every planted column"""
    from oracle import binding as ob
    c = S.case(name)
    res, off, gen, G = c.union(c.probe(n))
    ora = ob.Oracle(res, off, gen, S.K)
    out = ora.scores(G)
    ora.close()
    assert int(out["scoresCount"]) == c.n_col - 2
    return out


def _check_probe(nat, name, n, label):
    c = S.case(name)
    H.assert_scores_equal(nat.query_scores(*c.query(c.probe(n))).as_dict(), _want_probe(name, n), f"{label}: the probe row of {n} genes behind it")


@functools.lru_cache(maxsize=None)
def _kept():
    """the fixture the kept context goes back to, and a tiny query over its base with the oracle's answer"""
    from oracle import binding as ob
    fx, base, query, k, G = load_case("wide_row_9000_columns")
    rq, oq, _ = query.flatten()
    tiny = (np.frombuffer(b"CDEFGACDEF", np.uint8).copy(), np.array([0, 5, 10], np.uint64))       # (no AAA: no wide row)
    rb, ob_, gb = base.flatten()
    res = np.concatenate([rb, tiny[0]]); off = np.concatenate([ob_, ob_[-1] + tiny[1][1:]]).astype(np.uint64)
    gen = np.concatenate([gb, np.full(2, G, np.uint32)]).astype(np.uint32)
    ora = ob.Oracle(res, off, gen, k)
    want_tiny = ora.scores(G)
    ora.close()
    return fx, (rb, ob_, gb), (rq, oq), k, tiny, want_tiny


@pytest.fixture(scope="module")
def ctx():
    """ONE context for all single-query cases: its query buffers and HBM tables live from case to case"""
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.open()
    yield nat
    nat.close()


def _check_info(info, c, qs, label, chunks=1):
    """pdl_get_query_join_info of a call over the queries `qs` of case c against their plans; -> rows that left the LDS table"""
    lo = sum(c.expected_overflow(q)[0] for q in qs)
    hi = sum(c.expected_overflow(q)[1] for q in qs)
    may = sum(c.expected_may_overflow(q) for q in qs)
    print(f"{label}: {info}  (overflow rows planned {lo}..{hi}, may overflow {may})")
    assert info["rows"] == sum(len(c.queries[q]) for q in qs), label
    assert info["may_overflow_rows"] == may, label
    assert lo <= info["overflow_rows"] <= hi, label
    if chunks == 1:
        assert info["hbm_launches"] == (1 if info["overflow_rows"] else 0), label
        assert info["hbm_workgroups"] == min(info["overflow_rows"], S.QH_WG), label
    assert info["hbm_clears"] <= info["hbm_launches"] <= chunks, label
    return info["overflow_rows"]


def _check_kept(nat, label):
    fx, base, query, k, tiny, want_tiny = _kept()
    nat.preprocess(k, *base)
    assert_block(nat.query_scores(*query).as_dict(), fx, f"{label}: wide_row_9000_columns on the kept context")
    info = nat.last_query_join_info
    assert info["overflow_rows"] == 2 and info["hbm_workgroups"] == 2 and info["rows"] == 2, label
    H.assert_scores_equal(nat.query_scores(*tiny).as_dict(), want_tiny, f"{label}: a tiny query on the kept context")
    assert nat.last_query_join_info["overflow_rows"] == 0


@pytest.mark.parametrize("name", S.single_names())
def test_single_query_and_in_a_batch(name, ctx):
    c = S.case(name)
    nat = ctx
    nat.preprocess(S.K, *c.base)
    want, cost = _want(name, 0)
    got = nat.query_scores(*c.query(0)).as_dict()
    H.assert_scores_equal(got, want, f"{name}: pdl_query_scores")
    assert nat.last_query_info["genome_cost"] == cost, name
    over = _check_info(nat.last_query_join_info, c, [0], f"{name} single")
    # once more, on the tables and buffers the first run left (the same columns, the same slots: nothing is cleared)
    H.assert_scores_equal(nat.query_scores(*c.query(0)).as_dict(), want, f"{name}: pdl_query_scores again")
    again = nat.last_query_join_info
    _check_info(again, c, [0], f"{name} again")
    if over and again["overflow_rows"] <= over:
        assert again["hbm_clears"] == 0, f"{name}: clean tables of this layout were cleared again"
    # the probe: a cell in every planted column, on tables of the same layout (a column left dirty has none)
    n = len(c.queries[0])
    _check_probe(nat, name, n, f"{name} single")
    if over and c.n_col - 2 >= S.MUST_LEAVE:
        assert nat.last_query_join_info["hbm_clears"] == 0, f"{name}: the probe did not find the tables the case left"
    # the middle one of a batch
    (w0, q0), (w2, q2) = _want_small(name, 0), _want_small(name, 1)
    blocks = [b.as_dict() for b in nat.query_batch([q0, c.query(0), q2])]
    H.assert_scores_equal(blocks[1], want, f"{name}: pdl_query_batch, the planted query")
    H.assert_scores_equal(blocks[0], w0, f"{name}: pdl_query_batch, the query in front")
    H.assert_scores_equal(blocks[2], w2, f"{name}: pdl_query_batch, the query behind")
    assert nat.last_query_batch_info["queries"][1]["genome_cost"] == cost and nat.last_query_batch_info["chunks"] == 1
    info = nat.last_query_join_info
    assert info["rows"] == len(c.queries[0]) + 3 and info["may_overflow_rows"] == c.expected_may_overflow(0), name
    lo, hi = c.expected_overflow(0)
    assert lo <= info["overflow_rows"] <= hi and info["hbm_workgroups"] == min(info["overflow_rows"], S.QH_WG), name
    _check_probe(nat, name, max(n, 2), f"{name} batch")          # (the batch's tables: N + its largest query)
    _check_kept(nat, name)


@pytest.mark.parametrize("name", S.raw_names())
def test_the_fold_inside_a_wide_group_and_sums_near_2_to_the_20(name, ctx):
    """(and 341 rows that genes of their own query carry over the limit)  qextra, bextra, bskip where the group the union's fold changes has 3900 members (the tables in HBM) and 3000 (the LDS table);
    three cells whose 21-bit sums reach 2^20 - 2100, on the LDS table and on the tables in HBM"""
    c = S.raw_case(name)
    nat = ctx
    nat.preprocess(S.K, *c.base)
    want, cost = _want(name, 0)
    n = len(c.query_genes)
    for label in ("pdl_query_scores", "pdl_query_scores again"):
        H.assert_scores_equal(nat.query_scores(*c.query()).as_dict(), want, f"{name}: {label}")
        assert nat.last_query_info["genome_cost"] == cost, name
        over = _check_info(nat.last_query_join_info, c, [0], f"{name} {label}")
    assert over == c.expected_overflow()[0] and nat.last_query_join_info["hbm_clears"] == 0, name
    (w0, q0), (w2, q2) = _want_small(name, 0), _want_small(name, 1)
    blocks = [b.as_dict() for b in nat.query_batch([q0, c.query(), q2])]
    H.assert_scores_equal(blocks[1], want, f"{name}: pdl_query_batch, the planted query")
    H.assert_scores_equal(blocks[0], w0, f"{name}: pdl_query_batch, the query in front")
    H.assert_scores_equal(blocks[2], w2, f"{name}: pdl_query_batch, the query behind")
    info = nat.last_query_join_info
    assert info["rows"] == n + 3 and info["overflow_rows"] == over and info["may_overflow_rows"] == c.may_overflow, (name, info)
    H.assert_scores_equal(nat.query_scores(*c.query()).as_dict(), want, f"{name}: pdl_query_scores behind the batch")
    _check_kept(nat, name)


def test_the_read_out_at_the_limit(ctx):
    """what the issue asks of the read-out by name: LIMIT columns stay, LIMIT + QJ_T leave, 33 rows run on 16 workgroups"""
    for name, rows, wg in ((f"A-single-{S.QJ_LIMIT}", 0, 0), (f"A-spread-{S.QJ_LIMIT}", 0, 0), (f"A-single-{S.MUST_LEAVE}", 1, 1),
                           (f"A-spread-{S.MUST_LEAVE}", 1, 1), ("E-33-rows", 33, S.QH_WG), ("B-few", 0, 0)):
        c = S.case(name)
        ctx.preprocess(S.K, *c.base)
        H.assert_scores_equal(ctx.query_scores(*c.query(0)).as_dict(), _want(name, 0)[0], name)
        info = ctx.last_query_join_info
        assert (info["overflow_rows"], info["hbm_workgroups"], info["hbm_launches"]) == (rows, wg, 1 if rows else 0), (name, info)
        assert info["may_overflow_rows"] == (33 if rows == 33 else 1), (name, info)


@pytest.mark.parametrize("chunked", [False, True])
def test_tables_across_calls(chunked):
    from pandelos_amd.pangene_native import PangeneNative
    c = S.case("F-tables")
    nat = PangeneNative.open()
    nat.preprocess(S.K, *c.base)
    if chunked:
        nat.set_option("query_batch_bytes", 1)
    at = 0
    for step, (kind, queries, whole, per_query) in enumerate(S.table_steps()):
        qs = list(range(at, at + len(queries)))
        at += len(queries)
        label = f"step {step} ({kind}, {len(queries)} queries, chunked {chunked})"
        if kind == "single":
            blocks = [nat.query_scores(*c.query(qs[0])).as_dict()]
        else:
            blocks = [b.as_dict() for b in nat.query_batch([c.query(q) for q in qs])]
            assert nat.last_query_batch_info["chunks"] == (len(qs) if chunked else 1), label
        for q, b in zip(qs, blocks):
            H.assert_scores_equal(b, _want("F-tables", q)[0], f"{label}, query {q}")
        info = nat.last_query_join_info
        print(label, info)
        planted = sum(isinstance(r, S.QRow) for q in qs for r in c.queries[q])
        assert info["overflow_rows"] == info["may_overflow_rows"] == planted, (label, info)
        assert info["rows"] == sum(len(c.queries[q]) for q in qs), (label, info)
        assert (info["hbm_launches"], info["hbm_workgroups"], info["hbm_clears"]) == (per_query if chunked else whole), (label, info)
        if kind == "batch" or step % 2:                           # the probe, on tables of the step's layout
            n = max(len(c.queries[q]) for q in qs)
            _check_probe(nat, "F-tables", n, label)
            assert nat.last_query_join_info["hbm_clears"] == 0, f"{label}: the probe did not find the tables the step left"
    _check_kept(nat, "the table sequence")
    nat.close()


def test_33_rows_in_chunks(ctx):
    """the 33 rows as the middle query of a batch whose every query is a chunk of its own: the same blocks, the rows summed"""
    name = "E-33-rows"
    c = S.case(name)
    nat = ctx
    nat.preprocess(S.K, *c.base)
    (w0, q0), (w2, q2) = _want_small(name, 0), _want_small(name, 1)
    nat.set_option("query_batch_bytes", 1)
    try:
        blocks = [b.as_dict() for b in nat.query_batch([c.query(0), q0, c.query(0), q2])]
        assert nat.last_query_batch_info["chunks"] == 4
        info = nat.last_query_join_info
    finally:
        nat.set_option("query_batch_bytes", 1 << 30)
    for b, w in zip(blocks, (_want(name, 0)[0], w0, _want(name, 0)[0], w2)):
        H.assert_scores_equal(b, w, f"{name} in chunks")
    _check_probe(nat, name, 33, f"{name} in chunks")
    assert info["overflow_rows"] == info["may_overflow_rows"] == 66 and info["rows"] == 33 + 2 + 33 + 1, info
    assert info["hbm_launches"] == 2 and info["hbm_workgroups"] == S.QH_WG, info
    _check_kept(nat, name + " in chunks")


@pytest.mark.parametrize("name", PLACED)
def test_place_query_and_place_batch(name):
    """the edges of the placement are bbh_edges of the oracle's block, as tests/test_gpu_place.py compares them"""
    from pandelos_amd.pangene_native import PangeneNative
    from pandelos_amd.pangenes import bbh_edges
    from pandelos_amd.scores import Scores
    c = _case(name)
    want, cost = _want(name, 0)
    src, dst, score = bbh_edges(Scores(scoresCount=int(want["scoresCount"]), **{f: np.asarray(want[f]) for f in H.FIELDS}))
    nat = PangeneNative.open()
    nat.preprocess(S.K, *c.base)
    pl = nat.place_query(*c.query(0))
    over = _check_info(nat.last_query_join_info, c, [0], f"{name} place_query")
    assert over >= 1
    assert np.array_equal(pl["src"], src) and np.array_equal(pl["dst"], dst), f"{name}: pdl_place_query's edges differ from bbh_edges(oracle block)"
    assert H.raw(pl["score"]).tobytes() == H.raw(score).tobytes(), name
    assert nat.last_place_info["query"]["genome_cost"] == cost
    q0, q2 = _want_small(name, 0)[1], _want_small(name, 1)[1]
    pls = nat.place_batch([q0, c.query(0), q2])
    info = nat.last_query_join_info
    assert info["overflow_rows"] == over and info["rows"] == len(c.queries[0]) + 3, (name, info)
    assert np.array_equal(pls[1]["src"], src) and np.array_equal(pls[1]["dst"], dst), f"{name}: pdl_place_batch's edges differ from bbh_edges(oracle block)"
    assert H.raw(pls[1]["score"]).tobytes() == H.raw(score).tobytes(), name
    nat.close()


@pytest.mark.parametrize("sub,merged", SETTINGS)
def test_row_widths_into_k_order(sub, merged):
    """query rows that emit exactly 64, 65, 256, 257, 512, 513 cells, under every setting of K-order"""
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.open()
    nat.set_option("order_subwave", sub)
    nat.set_option("order_wide_merged", merged)
    for name in S.names_w():
        c = S.case(name)
        want, cost = _want(name, 0)
        assert int(want["scoresCount"]) == int(name.split("-")[1])
        nat.preprocess(S.K, *c.base)
        H.assert_scores_equal(nat.query_scores(*c.query(0)).as_dict(), want, f"{name}, order_subwave {sub}, merged {merged}")
        blocks = nat.query_batch([c.query(0), c.query(0)])
        for b in blocks:
            H.assert_scores_equal(b.as_dict(), want, f"{name} in a batch, order_subwave {sub}, merged {merged}")
    nat.close()


def test_refusal_at_2_to_the_20_k_mers_at_all_four_doors():
    """a query gene of exactly 2^20 k-mers is refused by each of the four (the guard in front of the accumulator's 21-bit fields),
    and the context answers the next query as before"""
    from pandelos_amd import _lib
    from pandelos_amd.pangene_native import PangeneNative
    c = S.case("W-64-cells")
    nat = PangeneNative.open()
    nat.preprocess(S.K, *c.base)
    before = nat.query_scores(*c.query(0)).as_dict()
    info = nat.last_query_join_info
    n = S.GENE_KMERS_GUARD + S.K - 1
    long_gene = (np.resize(c.query(0)[0], n).astype(np.uint8), np.array([0, n], np.uint64))
    for call in (lambda: nat.query_scores(*long_gene), lambda: nat.query_batch([c.query(0), long_gene]),
                 lambda: nat.place_query(*long_gene), lambda: nat.place_batch([c.query(0), long_gene])):
        with pytest.raises(_lib.PdlError) as e:
            call()
        assert e.value.code == _lib.PDL_ERR_UNSUPPORTED and "2^20" in str(e.value), str(e.value)
        assert nat.last_query_join_info == info                   # (the report is of the last SUCCESSFUL call)
    H.assert_scores_equal(nat.query_scores(*c.query(0)).as_dict(), before, "after the refusals")
    nat.close()
