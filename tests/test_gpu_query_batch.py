"""pdl_query_batch on the GPU: q new genomes against an existing dictionary in one pass, each block bit for bit the one
pdl_query_scores returns for that genome alone — against the reference fixtures, the single query, and the CPU oracle on
base + that genome; the queries never see each other; the base context left as it was; chunking; the refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import helpers as H
from tests.test_gpu_query import _check_against_oracle, _genes, _native, _union
from tests.test_query_golden import CASES, assert_block, load_case

pytestmark = pytest.mark.gpu
N_SEEDS = int(os.environ.get("PDL_QUERY_BATCH_SEEDS", "120"))


def _groups():
    """The fixture cases grouped by identical base and k: {(base bytes, k): [names]}."""
    groups = {}
    for name in CASES:
        fx = dict(np.load(H.GOLDEN / "query" / f"{name}.npz"))
        groups.setdefault((fx["base_faa"].tobytes(), int(fx["k"])), []).append(name)
    return sorted(groups.values())


GROUPS = _groups()


Q1 = [n for n in CASES if n.startswith("q1")]


def _fold_case(base, query, k):
    """The case of DESIGN.md §9's Q1 a query falls into against a base, worked out on the host.  A polynomial rank orders
    k-mers as their bytes do (the rank table is dense in byte order), so byte strings stand in for ranks: bmax / r2 = the
    base's largest / second k-mer, lonely = one base record holds bmax (the base folded it), qmax = the query's largest,
    alone = one query gene holds it.  '-' = no fold is touched."""
    def records(data):
        out = {}
        for g, s in enumerate(data.sequences):
            for i in range(len(s) - k + 1):
                out.setdefault(bytes(s[i:i + k]), set()).add(g)
        return out
    b, q = records(base), records(query)
    ranks = sorted(b)
    bmax, r2 = ranks[-1], (ranks[-2] if len(ranks) > 1 else None)
    lonely = len(b[bmax]) == 1 and sum(len(v) for v in b.values()) > 1
    qmax = max(q)
    if qmax > bmax:
        return "a" if len(q[qmax]) == 1 else ("b" if lonely else "-")
    if qmax == bmax:
        return "b" if lonely else "d"
    return "c" if lonely and (r2 is None or qmax > r2) else "-"


@pytest.mark.parametrize("name", Q1)
def test_fold_cases_coexist_in_one_batch(name):
    """The q1a..q1d fixtures (cases (a)-(d) of the union's last-record fold) each have a base of their own, so grouping by base
    leaves them batches of one.  Here every q1 base gets ALL the q1 queries its alphabet allows in one batch: queries in
    different fold cases side by side, each against the single query and the oracle, the base's own query against its fixture."""
    from pandelos_amd.pangene_native import PangeneNative
    assert len(Q1) == 4
    fx, base, own, k, G = load_case(name)
    res_b, off_b, gen_b = base.flatten()
    letters = np.unique(res_b)
    names = [n for n in Q1 if np.isin(load_case(n)[2].flatten()[0], letters).all()]
    assert name in names and len(names) >= 3, names
    queries = [load_case(n)[2].flatten()[:2] for n in names]
    cases = [_fold_case(base, load_case(n)[2], k) for n in names]
    assert cases[names.index(name)] == name[2], (name, cases)         # q1a is case (a) on its own base, ...
    assert len(set(cases)) >= 2, (names, cases)                       # ... and the batch holds queries in different cases
    nat = PangeneNative(k, base)
    blocks = nat.query_batch(queries + queries[::-1])
    for j, (n, q, block) in enumerate(zip(names + names[::-1], queries + queries[::-1], blocks)):
        got = block.as_dict()
        if n == name:
            assert_block(got, fx, f"{name}: its own query in the batch")
        H.assert_scores_equal(got, nat.query_scores(*q).as_dict(), f"base of {name}, query of {n}")
        _check_against_oracle(nat, (res_b, off_b, gen_b), q, k, f"base of {name}, query of {n}")
    nat.close()


@pytest.mark.parametrize("names", GROUPS, ids=lambda g: "+".join(g))
def test_reference_fixtures_as_one_batch(names):
    from pandelos_amd.pangene_native import PangeneNative
    cases = [load_case(n) for n in names]
    _, base, _, k, _ = cases[0]
    nat = PangeneNative(k, base)
    blocks = nat.query_batch_idata([c[2] for c in cases])
    assert len(blocks) == len(names)
    info = nat.last_query_batch_info
    for name, (fx, _, _, _, G), block, qi in zip(names, cases, blocks, info["queries"]):
        got = block.as_dict()
        assert_block(got, fx, name)
        assert (np.asarray(got["first_seq_genome"]) == G).all()
        assert qi["genome_cost"] == int(fx["genome_cost"]), name
        assert qi["kmer_occurrences"] >= qi["records"] >= qi["matched_records"]
    assert info["chunks"] >= 1
    nat.close()


# ---- random small sets ---------------------------------------------------------------------------------------------------
def _pack(genes):
    off = np.zeros(len(genes) + 1, np.uint64)
    np.cumsum([len(g) for g in genes], out=off[1:])
    res = np.concatenate(genes).astype(np.uint8) if genes else np.zeros(0, np.uint8)
    return res, off


def _random_batch_case(seed):
    """A usable case for every seed: the draw is repeated with a sub-seed until the base has a k-mer and a held-out genome
    uses the base's letters only."""
    for sub in range(64):
        case = _draw_batch_case(seed + 100_000 * sub)
        if case is not None:
            return case
    raise AssertionError(f"seed {seed}: no usable split in 64 draws")


def _draw_batch_case(seed):
    """-> (base arrays, [query arrays], k): 2-6 genomes held out of a random small set, plus a query of one gene, a query
    whose genes are all shorter than k, and a second copy of the first query; None when the draw cannot be used."""
    from tests.test_gpu_fuzz import _random_set
    res, off, _, k = _random_set(seed)
    off = off.astype(np.int64)
    genes = [res[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    rng = np.random.default_rng(seed ^ 0x5eed)
    n_held = int(rng.integers(2, 7))
    n_base = int(rng.integers(1, 5))
    gid = rng.integers(0, n_base + n_held, len(genes))
    base_genes, base_gen, seen = [], [], {}
    for g, x in zip(genes, gid):
        if x < n_base:
            base_genes.append(g)
            base_gen.append(seen.setdefault(int(x), len(seen)))
    if not base_genes or not any(len(g) >= k for g in base_genes):
        return None                                                   # (no base k-mer: undefined in the reference)
    rb, ob_ = _pack(base_genes)
    letters = np.unique(rb)
    queries = []
    for h in range(n_base, n_base + n_held):
        qg = [g for g, x in zip(genes, gid) if x == h]
        if qg and np.isin(np.concatenate(qg), letters).all():        # (a letter the base lacks is refused: tested below)
            queries.append(_pack(qg))
    if not queries:
        return None
    first = queries[0]
    one = [g for g in base_genes if len(g) >= k][0]
    queries.append(_pack([one[: max(k, len(one) // 2)]]))             # one gene
    queries.append(_pack([rb[: max(0, k - 1)], rb[:0], rb[1: k]]))    # genes shorter than k only (one of them empty)
    queries.append((first[0].copy(), first[1].copy()))                # the first query again
    return (rb, ob_, np.asarray(base_gen, np.uint32)), queries, k


@pytest.mark.parametrize("seed", list(range(7000, 7000 + N_SEEDS)))
def test_random_small_sets_match_the_single_query_and_the_oracle(seed):
    from oracle import binding as ob
    base, queries, k = _random_batch_case(seed)
    nat = _native(k, *base)
    blocks = [b.as_dict() for b in nat.query_batch(queries)]
    infos = nat.last_query_batch_info["queries"]
    assert len(blocks) == len(queries) == len(infos)
    for j, (query, got, qi) in enumerate(zip(queries, blocks, infos)):
        label = f"seed {seed} query {j}"
        single = nat.query_scores(*query).as_dict()
        H.assert_scores_equal(got, single, label + " vs single")
        assert qi["genome_cost"] == nat.last_query_info["genome_cost"], label
        for f in ("residues", "kmer_occurrences", "records", "matched_records"):
            assert qi[f] == nat.last_query_info[f], (label, f)
        res, off, gen, G = _union(base, query)
        ora = ob.Oracle(res, off, gen, k)
        H.assert_scores_equal(got, ora.scores(G), label + " vs oracle")
        assert qi["genome_cost"] == ora.genome_cost(G), label
        assert np.asarray(got["max_genome_score"]).shape == (len(query[1]) - 1, G + 1) and len(got["max_genome_score_col"]) == len(gen), label
    H.assert_scores_equal(blocks[-1], blocks[0], f"seed {seed}: identical queries")     # neither saw the other
    nat.close()


def test_mid_size_eight_held_out_genomes():
    """The 64 x 750 x 370 protein-like set minus its last 8 genomes; the 8 in one batch, each against the oracle on base + it."""
    from oracle import binding as ob
    from pandelos_amd.synth import make_gene_set
    gs = make_gene_set(genomes=64, genes_per_genome=750, mean_len=370, sub_rate=0.25, seed=6465, protein_like=True)
    off = gs.offsets.astype(np.int64)
    gen = gs.genome_of

    def cut(sel):
        idx = np.flatnonzero(sel)
        assert (np.diff(idx) == 1).all()                              # (the synthetic set is genome major)
        lo, hi = int(off[idx[0]]), int(off[idx[-1] + 1])
        return gs.residues[lo:hi].copy(), (off[idx[0]:idx[-1] + 2] - lo).astype(np.uint64)
    rb, ob_ = cut(gen < 56)
    base = (rb, ob_, gen[gen < 56].astype(np.uint32))
    queries = [cut(gen == g) for g in range(56, 64)]
    nat = _native(5, *base)
    blocks = nat.query_batch(queries)
    assert nat.last_query_batch_info["chunks"] == 1
    for j, (query, block) in enumerate(zip(queries, blocks)):
        res, o, g, G = _union(base, query)
        ora = ob.Oracle(res, o, g, 5)
        H.assert_scores_equal(block.as_dict(), ora.scores(G), f"56+1, query {j}")
        assert nat.last_query_batch_info["queries"][j]["genome_cost"] == ora.genome_cost(G)
        del ora
    nat.close()


def test_wide_rows_in_a_batch_then_a_single_query_then_another_batch():
    """Rows that leave the LDS table use HBM tables laid out for N + the batch's largest query; a single query and a batch of
    other sizes afterwards must find tables they can trust (the hbm_cols bookkeeping)."""
    from oracle import binding as ob
    fx, base, query, k, G = load_case("wide_row_9000_columns")
    res_b, off_b, gen_b = base.flatten()
    b = (res_b, off_b, gen_b)
    wide = query.flatten()[:2]
    nat = _native(k, res_b, off_b, gen_b)

    def check(queries, label):
        for j, (q, block) in enumerate(zip(queries, nat.query_batch(queries))):
            res, off, gen, g_union = _union(b, q)
            H.assert_scores_equal(block.as_dict(), ob.Oracle(res, off, gen, k).scores(g_union), f"{label}, query {j}")
        return

    first = [_genes(b"AAAA", b"CDEFAAA", b"AAAD", b"KLAAAC"), wide, _genes(b"ACDEF"), _genes(b"AAAC", b"ACDEF", b"AAAK", b"EFG", b"AAAAA", b"HIKAAA")]
    check(first, "first batch")
    blocks = nat.query_batch(first)
    assert_block(blocks[1].as_dict(), fx, "the fixture's query inside the batch")
    assert int((np.asarray(blocks[1].row) == np.asarray(blocks[1].row)[0]).sum()) > 8192
    assert_block(nat.query_idata(query).as_dict(), fx, "single query after the batch")
    _check_against_oracle(nat, b, first[0], k, "single query of four genes")
    check([wide, _genes(b"AAAK", b"AAAE", b"AAAF")], "second batch, other sizes")
    check([_genes(b"AAAK"), wide, wide], "third batch")
    assert_block(nat.query_idata(query).as_dict(), fx, "single query at the end")
    nat.close()


def test_chunking_does_not_change_the_blocks():
    from pandelos_amd.synth import make_gene_set
    gs = make_gene_set(genomes=10, genes_per_genome=60, mean_len=90, sub_rate=0.1, seed=314)
    off = gs.offsets.astype(np.int64)
    gen = gs.genome_of
    genes = [gs.residues[off[i]:off[i + 1]] for i in range(len(gen))]
    rb, ob_ = _pack([g for g, x in zip(genes, gen) if x < 4])
    base = (rb, ob_, gen[gen < 4].astype(np.uint32))
    queries = [_pack([g for g, x in zip(genes, gen) if x == h]) for h in range(4, 10)]
    nat = _native(3, *base)
    whole = [b.as_dict() for b in nat.query_batch(queries)]
    assert nat.last_query_batch_info["chunks"] == 1
    def run(budget):
        nat.set_option("query_batch_bytes", budget)
        parts = [b.as_dict() for b in nat.query_batch(queries)]
        chunks = nat.last_query_batch_info["chunks"]
        for j, (x, y) in enumerate(zip(parts, whole)):
            H.assert_scores_equal(x, y, f"budget {budget}: {chunks} chunks, query {j}")
        assert [q["genome_cost"] for q in nat.last_query_batch_info["queries"]] == costs, budget
        return chunks
    costs = _costs(nat, queries)
    assert run(1) == 6                                                # a chunk of one query works whatever the budget
    # chunks of SEVERAL queries that start past query 0: a query weighs about half a megabyte here (~5.3 k k-mers x ~100 bytes),
    # so some budget between 0.6 and 3 MB cuts the six into three chunks (a chunk takes all the consecutive queries that fit,
    # so three chunks of six near-equal queries cannot be 4 + 1 + 1: a later chunk holds more than one)
    seen = {}
    for budget in range(600_000, 3_000_000, 50_000):
        seen[budget] = run(budget)
        if seen[budget] <= 3:
            break
    assert 3 in seen.values(), seen
    assert all(a >= b for a, b in zip(list(seen.values()), list(seen.values())[1:])), seen      # a larger budget never gives more chunks
    nat.set_option("query_batch_bytes", 1 << 30)
    again = [b.as_dict() for b in nat.query_batch(queries)]
    assert nat.last_query_batch_info["chunks"] == 1
    for x, y in zip(again, whole):
        H.assert_scores_equal(x, y, "default budget again")
    with pytest.raises(Exception):
        nat.set_option("query_batch_bytes", 0)
    nat.close()


def _costs(nat, queries):
    out = []
    for q in queries:
        nat.query_scores(*q)
        out.append(nat.last_query_info["genome_cost"])
    return out


def test_canonical_order_and_a_genome_shard():
    from pandelos_amd import _lib
    fx, base, query, k, G = load_case("protein_like_held_out")
    res_b, off_b, gen_b = base.flatten()
    q = query.flatten()[:2]
    half = (q[0][: int(q[1][len(q[1]) // 2])].copy(), q[1][: len(q[1]) // 2 + 1].copy())
    nat = _native(k, res_b, off_b, gen_b, flags=_lib.PDL_FLAG_CANONICAL_ORDER, shard=[0, 2])
    blocks = [b.as_dict() for b in nat.query_batch([half, q, half])]
    order = np.lexsort((fx["column"], fx["row"]))
    for f in ("scores", "percs", "tr_percs", "row", "column"):
        assert np.array_equal(H.raw(blocks[1][f]), fx[f][order]), f
    for f in ("max_genome_score", "max_genome_score_col", "scoresMaxMappings"):
        assert np.array_equal(H.raw(blocks[1][f]), fx[f]), f
    H.assert_scores_equal(blocks[0], nat.query_scores(*half).as_dict(), "canonical half")
    H.assert_scores_equal(blocks[2], blocks[0], "identical queries")
    nat.close()
    plain = _native(k, res_b, off_b, gen_b, shard=[0, 2])
    assert_block(plain.query_batch([half, q])[1].as_dict(), fx, "shard")
    plain.close()


def _snapshot(nat, G):
    return {"scores": [nat.generate_scores_part(g).as_dict() for g in range(G)], "edges": [nat.generate_edges_part(g) for g in range(G)],
            "dictionary": nat.dictionary(), "costs": [nat.genome_cost(g) for g in range(G)], "cost": nat.cost.as_dict(),
            "timings": nat.timings(), "families": nat.generate_families()}


def _assert_snapshot(nat, G, before, label):
    after = _snapshot(nat, G)
    for g in range(G):
        H.assert_scores_equal(after["scores"][g], before["scores"][g], f"{label}: base genome {g}")
        assert all(np.array_equal(x, y) for x, y in zip(after["edges"][g], before["edges"][g])), (label, g)
    assert all(np.array_equal(x, y) for x, y in zip(after["dictionary"], before["dictionary"])), label
    assert after["costs"] == before["costs"] and after["cost"] == before["cost"], label
    assert after["timings"] == before["timings"], label
    fa, fb = after["families"], before["families"]
    assert fa.keys() == fb.keys()
    for key in fa:
        assert np.array_equal(fa[key], fb[key]), (label, key)


def test_the_base_context_is_left_as_it_was():
    fx, base, query, k, G = load_case("protein_like_held_out")
    res_b, off_b, gen_b = base.flatten()
    q = query.flatten()[:2]
    nat = _native(k, res_b, off_b, gen_b)
    before = _snapshot(nat, G)
    a = nat.query_batch([q, _genes(b"ACDEFGHIK"), q])
    b = nat.query_batch([q])
    assert_block(a[0].as_dict(), fx, "first batch")
    assert_block(b[0].as_dict(), fx, "second batch")
    _assert_snapshot(nat, G, before, "after two batches")
    nat.close()


def test_refusals():
    from pandelos_amd import _lib
    from pandelos_amd.pangene_native import PangeneNative
    fx, base, query, k, G = load_case("identical_gene")
    res_b, off_b, gen_b = base.flatten()
    rq, oq, _ = query.flatten()
    good = (rq, oq)

    def code(fn):
        with pytest.raises(_lib.PdlError) as e:
            fn()
        return e.value.code, str(e.value)

    # the states pdl_query_scores refuses
    fresh = PangeneNative.open()
    assert code(lambda: fresh.query_batch([good]))[0] == _lib.PDL_ERR_STATE
    fresh.close()
    cplx = PangeneNative.from_arrays(k, res_b, off_b, gen_b, only_complexity=True)
    assert code(lambda: cplx.query_batch([good]))[0] == _lib.PDL_ERR_STATE
    cplx.close()
    low = PangeneNative.open()
    low.set_option("low_memory", 1)
    low.preprocess(k, res_b, off_b, gen_b)
    assert code(lambda: low.query_batch([good]))[0] == _lib.PDL_ERR_STATE
    low.close()

    nat = _native(k, res_b, off_b, gen_b)
    before = _snapshot(nat, G)
    res, off, begin = PangeneNative.pack_queries([good, good, good, good])
    n, q = len(off) - 1, 4

    def raw(res=res, off=off, begin=begin, n=n, q=q, out=True, null_res=False):
        blocks = (_lib.PdlScores * 4)()
        for b in blocks:                                              # stale values: a refusal must leave `out` zeroed
            b.scoresCount, b.rows = 77, 88
        infos = (_lib.PdlQueryInfo * 4)()
        binfo = _lib.PdlQueryBatchInfo()
        rc = nat._lib.pdl_query_batch(nat._ctx, None if null_res else res.ctypes.data, None if off is None else off.ctypes.data,
                                      None if begin is None else begin.ctypes.data, n, q, blocks if out else None, infos, C.byref(binfo))
        if rc != _lib.PDL_OK and out:
            for b in blocks[:q]:
                assert bytes(b) == bytes(C.sizeof(_lib.PdlScores)), "out is not zeroed after a refusal"
        if rc == _lib.PDL_OK:
            for b in blocks:
                nat._lib.pdl_free_scores(C.byref(b))
        return rc, nat._lib.pdl_last_error(nat._ctx).decode()

    assert raw()[0] == _lib.PDL_OK
    A, U = _lib.PDL_ERR_ARGUMENT, _lib.PDL_ERR_UNSUPPORTED
    assert raw(q=0)[0] == A
    assert raw(n=0, begin=np.zeros(5, np.uint32))[0] == A
    assert raw(off=None)[0] == A and raw(begin=None)[0] == A and raw(out=False)[0] == A and raw(null_res=True)[0] == A
    bad_off = off.copy(); bad_off[2] = bad_off[1] - 1
    assert raw(off=bad_off)[0] == A
    u32 = lambda *v: np.array(v, np.uint32)
    per = int(begin[1])
    assert raw(begin=u32(1, per, 2 * per, 3 * per, n))[0] == A                 # does not start at 0
    assert raw(begin=u32(0, per, 2 * per, 3 * per, n - 1))[0] == A             # does not end at n (or, with one gene each, an empty query)
    assert raw(begin=u32(0, per, 2 * per, 3 * per, n + 1))[0] == A             # ends past n
    assert raw(begin=u32(0, per, per, 3 * per, n))[0] == A                     # a query without genes
    assert raw(begin=u32(0, 2 * per, per, 3 * per, n))[0] == A                 # decreasing
    # bytes the base lacks in query 2 of 4 (and a smaller one in query 3): the first such query and ITS smallest absent byte
    z = (np.frombuffer(b"ACAZZX", np.uint8).copy(), np.array([0, 6], np.uint64))
    z3 = (np.frombuffer(b"ACAB", np.uint8).copy(), np.array([0, 4], np.uint64))
    c, msg = code(lambda: nat.query_batch([good, good, z, z3]))
    assert c == U and "query 2" in msg and "0x58" in msg and "'X'" in msg, msg
    nat.set_option("query_batch_bytes", 1)                            # ... also when earlier chunks had their blocks made
    c, msg = code(lambda: nat.query_batch([good, good, z, z3]))
    assert c == U and "query 2" in msg and "0x58" in msg, msg
    r4, o4, b4 = PangeneNative.pack_queries([good, good, z, z3])
    rc, msg = raw(res=r4, off=o4, begin=b4, n=len(o4) - 1)
    assert rc == U and "query 2" in msg
    nat.set_option("query_batch_bytes", 1 << 30)
    # a gene of 2^20 k-mers or more
    long_gene = (np.resize(rq, (1 << 20) + k + 3).astype(np.uint8), np.array([0, (1 << 20) + k + 3], np.uint64))
    c, msg = code(lambda: nat.query_batch([good, long_gene]))
    assert c == U and "2^20" in msg and "query 1" in msg, msg
    _assert_snapshot(nat, G, before, "after the refusals")
    assert_block(nat.query_batch([good])[0].as_dict(), fx, "after refusals")
    with pytest.raises(ValueError):
        from pandelos_amd.pangene_idata import PangeneIData
        nat.query_batch_idata([PangeneIData.from_arrays(rq, oq[:3], np.array([0, 1], np.uint32))])
    nat.close()


def test_multi_gpu_context_is_refused():
    import torch
    from pandelos_amd import _lib
    from pandelos_amd.pangene_native import PangeneNative
    fx, base, query, k, G = load_case("identical_gene")
    res_b, off_b, gen_b = base.flatten()
    rq, oq, _ = query.flatten()
    dev = torch.device("cuda", 0)
    t_res = torch.from_numpy(np.concatenate([res_b, np.zeros(32, np.uint8)])).to(dev)
    t_off = torch.from_numpy(off_b.astype(np.int64)).to(dev)
    t_gen = torch.from_numpy(gen_b.astype(np.int32)).to(dev)
    nat = PangeneNative.open()
    nat.dist_preprocess_begin(k, t_res.data_ptr(), t_off.data_ptr(), t_gen.data_ptr(), len(gen_b), len(res_b), 1, 0)
    with pytest.raises(_lib.PdlError) as e:
        nat.query_batch([(rq, oq)])
    assert e.value.code == _lib.PDL_ERR_STATE
    nat.close()


def test_size_limits_are_refused_from_the_offsets_and_gene_begin_alone():
    """Residues past 2^32 are decided from the offsets (the residues pointer is not followed before the refusal), N + n_j past
    the 31-bit ids from gene_begin, before offsets is read — so no array of 2^31 offsets has to exist to see that refusal."""
    from pandelos_amd import _lib
    fx, base, query, k, G = load_case("identical_gene")
    res_b, off_b, gen_b = base.flatten()
    nat = _native(k, res_b, off_b, gen_b)
    blocks = (_lib.PdlScores * 2)()
    dummy = np.zeros(16, np.uint8)
    off = np.array([0, 8, 1 << 32], np.uint64)
    rc = nat._lib.pdl_query_batch(nat._ctx, dummy.ctypes.data, off.ctypes.data, np.array([0, 1, 2], np.uint32).ctypes.data, 2, 2, blocks, None, None)
    assert rc == _lib.PDL_ERR_UNSUPPORTED and "2^32" in nat._lib.pdl_last_error(nat._ctx).decode()
    assert bytes(blocks[0]) == bytes(C.sizeof(_lib.PdlScores))
    n = 0x7fffffff - len(gen_b) + 1
    begin = np.array([0, 1, n], np.uint32)                            # query 1 is the one past the limit
    rc = nat._lib.pdl_query_batch(nat._ctx, dummy.ctypes.data, off.ctypes.data, begin.ctypes.data, n, 2, blocks, None, None)
    msg = nat._lib.pdl_last_error(nat._ctx).decode()
    assert rc == _lib.PDL_ERR_UNSUPPORTED and "31-bit gene ids" in msg and "query 1" in msg, msg
    assert bytes(blocks[0]) == bytes(C.sizeof(_lib.PdlScores)) and bytes(blocks[1]) == bytes(C.sizeof(_lib.PdlScores))
    assert_block(nat.query_batch([query.flatten()[:2]])[0].as_dict(), fx, "after the size refusals")
    nat.close()


def test_query_batch_command_end_to_end(tmp_path):
    from pandelos_amd import query as Q
    from pandelos_amd import query_batch as QB
    fx, base, query, k, G = load_case("protein_like_held_out")
    bf = tmp_path / "base.faa"
    bf.write_bytes(fx["base_faa"].tobytes())
    # three query genomes in two files: the fixture's genome whole, and two halves of it under labels of their own
    recs = list(zip(query.sequenceName, query.sequenceDescription, query.sequences))
    half = len(recs) // 2

    def faa(label, part):
        return b"".join(f"{label}\t{n}\t{d}\n".encode("latin-1") + s + b"\n" for n, d, s in part)
    label = query.genomeNames[0]
    singles = {label: faa(label, recs), "left_half": faa("left_half", recs[:half]), "right-half.2": faa("right-half.2", recs[half:])}
    f1, f2 = tmp_path / "q1.faa", tmp_path / "q2.faa"
    # genomes interleaved inside a file: first-seen order, genes in file order
    inter = b"".join(faa(label, [a]) + faa("left_half", [b]) for a, b in zip(recs[:half], recs[:half])) + faa(label, recs[half:])
    f1.write_bytes(inter)
    f2.write_bytes(singles["right-half.2"])
    out = tmp_path / "out"
    assert QB.main(["-i", str(bf), "-k", str(k), "-q", str(f1), "-q", str(f2), "--out-dir", str(out), "--cells"]) == 0
    assert sorted(p.name for p in out.iterdir()) == sorted([f"{x}.net" for x in singles] + [f"{x}.tsv" for x in singles])
    for name, data in singles.items():
        qf, net, cells = tmp_path / f"single_{name}.faa", tmp_path / f"single_{name}.net", tmp_path / f"single_{name}.tsv"
        qf.write_bytes(data)
        assert Q.main(["-i", str(bf), "-k", str(k), "-q", str(qf), "-o", str(net), "--cells", str(cells)]) == 0
        assert (out / f"{name}.net").read_bytes() == net.read_bytes(), name
        assert (out / f"{name}.tsv").read_bytes() == cells.read_bytes(), name
    assert (out / f"{label}.net").stat().st_size > 0
