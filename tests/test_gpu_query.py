"""pdl_query_scores on the GPU: one new genome against an existing dictionary, bit for bit against the block the reference
(fixtures) and the CPU oracle return for genome G of the union run; the base context left as it was; the refusals."""
import os

import numpy as np
import pytest

from tests import helpers as H
from tests.test_query_golden import CASES, assert_block, load_case, union_arrays

pytestmark = pytest.mark.gpu
N_SEEDS = int(os.environ.get("PDL_QUERY_SEEDS", "120"))


def _native(k, res, off, gen, flags=0, options=(), shard=None, late=()):
    """`late`: options set on the built context, behind one scoring pass (tests/option_forms.py)."""
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.open(flags=flags)
    for name, v in options:
        nat.set_option(name, v)
    if shard is not None:
        nat.set_genome_shard(shard)
    nat.preprocess(k, res, off, gen)
    if late:
        nat.score_all()
        for name, v in late:
            nat.set_option(name, v)
    return nat


def _split(res, off, gen, held):
    """(base arrays, query arrays) with the genes of genome `held` as the query; base ids stay dense (first-seen order)."""
    off = off.astype(np.int64)
    genes = [res[off[i]:off[i + 1]] for i in range(len(gen))]
    bi = [i for i in range(len(gen)) if gen[i] != held]
    qi = [i for i in range(len(gen)) if gen[i] == held]

    def pack(ids):
        o = np.zeros(len(ids) + 1, np.uint64)
        np.cumsum([len(genes[i]) for i in ids], out=o[1:])
        r = np.concatenate([genes[i] for i in ids]) if ids else np.zeros(0, np.uint8)
        return r.astype(np.uint8), o
    rb, ob_ = pack(bi)
    gb = gen[bi].astype(np.int64)
    remap = {}
    for x in gb:
        remap.setdefault(int(x), len(remap))
    gb = np.array([remap[int(x)] for x in gb], np.uint32)
    rq, oq = pack(qi)
    return (rb, ob_, gb), (rq, oq)


def _union(base, query):
    (rb, ob_, gb), (rq, oq) = base, query
    G = int(gb.max()) + 1
    res = np.concatenate([rb, rq]).astype(np.uint8)
    off = np.concatenate([ob_, ob_[-1] + oq[1:]]).astype(np.uint64)
    gen = np.concatenate([gb, np.full(len(oq) - 1, G, np.uint32)])
    return res, off, gen, G


def _check_against_oracle(nat, base, query, k, label, ora=None):
    """`ora`: the oracle on the union where the caller has it already"""
    from oracle import binding as ob
    res, off, gen, G = _union(base, query)
    ora = ora or ob.Oracle(res, off, gen, k)
    got = nat.query_scores(*query).as_dict()
    H.assert_scores_equal(got, ora.scores(G), label)
    assert nat.last_query_info["genome_cost"] == ora.genome_cost(G), label
    assert (got["first_seq_genome"] == G).all()
    return got, ora


@pytest.mark.parametrize("name", CASES)
def test_fixture(name):
    fx, base, query, k, G = load_case(name)
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative(k, base)
    got = nat.query_idata(query).as_dict()
    assert_block(got, fx, name)
    info = nat.last_query_info
    assert info["genome_cost"] == int(fx["genome_cost"])
    assert info["kmer_occurrences"] >= info["records"] >= info["matched_records"]
    nat.close()


def test_wide_row_leaves_the_lds_table_and_stays_exact():
    fx, base, query, k, G = load_case("wide_row_9000_columns")
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative(k, base)
    got = nat.query_idata(query).as_dict()
    assert_block(got, fx, "wide row")
    assert int((np.asarray(got["row"]) == np.asarray(got["row"])[0]).sum()) > 8192


def _genes(*seqs):
    res = np.frombuffer(b"".join(seqs), np.uint8).copy()
    off = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(x) for x in seqs], out=off[1:])
    return res, off


def test_queries_of_other_sizes_in_turn_keep_the_wide_rows_exact():
    """Rows that leave the LDS table use tables in HBM laid out by the union's column count N + n: queries of different gene
    counts on ONE context (more genes, fewer, more again), each with rows of 9000 columns, must all stay exact."""
    fx, base, query, k, G = load_case("wide_row_9000_columns")
    res_b, off_b, gen_b = base.flatten()
    nat = _native(k, res_b, off_b, gen_b)
    b = (res_b, off_b, gen_b)
    _check_against_oracle(nat, b, _genes(b"AAAA", b"CDEFAAA", b"AAAD", b"KLAAAC"), k, "four genes")
    assert_block(nat.query_idata(query).as_dict(), fx, "two genes after four")
    _check_against_oracle(nat, b, _genes(b"AAAC", b"ACDEF", b"AAAK", b"EFG", b"AAAAA", b"HIKAAA"), k, "six genes after two")
    _check_against_oracle(nat, b, _genes(b"ACDEF"), k, "one gene, no wide row")
    assert_block(nat.query_idata(query).as_dict(), fx, "two genes again")
    nat.close()


def test_short_and_empty_query_genes():
    from pandelos_amd.synth import make_gene_set
    gs = make_gene_set(genomes=4, genes_per_genome=30, mean_len=60, sub_rate=0.1, seed=77)
    base, query = _split(gs.residues, gs.offsets, gs.genome_of, int(gs.genome_of.max()))
    rq, oq = query
    extra = [np.zeros(0, np.uint8), rq[:2], rq[:3]]                 # an empty gene, genes shorter than / as long as k
    rq = np.concatenate([rq] + extra).astype(np.uint8)
    oq = np.concatenate([oq, oq[-1] + np.cumsum([len(e) for e in extra])]).astype(np.uint64)
    nat = _native(3, *base)
    _check_against_oracle(nat, base, (rq, oq), 3, "short/empty")
    # a query with no k-mer at all: an empty block of the right shape
    q0 = (rq[:2].copy(), np.array([0, 0, 2], np.uint64))
    got, _ = _check_against_oracle(nat, base, q0, 3, "no k-mer")
    assert got["scoresCount"] == 0 and got["max_genome_score"].shape == (2, int(base[2].max()) + 2)


def _random_case(seed):
    from tests.test_gpu_fuzz import _random_set
    res, off, gen, k = _random_set(seed)
    if gen.max(initial=0) < 1:
        return None
    held = int(gen.max())
    base, query = _split(res, off, gen, held)
    rb, ob_, _ = base
    if int((np.diff(ob_.astype(np.int64)) >= k).sum()) == 0:
        return None                                                   # (no base k-mer: undefined in the reference)
    if not np.isin(query[0], rb).all():
        return None                                                   # a letter the base lacks: refused (tested below)
    return base, query, k


@pytest.mark.parametrize("seed", list(range(5000, 5000 + N_SEEDS)))
def test_random_small_sets_match_the_oracle(seed):
    case = _random_case(seed)
    if case is None:
        pytest.skip("seed gives no usable split")
    base, query, k = case
    nat = _native(k, *base)
    got, ora = _check_against_oracle(nat, base, query, k, f"seed {seed}")
    got2 = nat.query_scores(*query).as_dict()                        # queries are independent of each other
    H.assert_scores_equal(got2, got, f"seed {seed} repeat")
    nat.close()


@pytest.mark.parametrize("seed,tier,tier0,protein", [(61, 10, 0, False), (62, 11, 1, True), (63, 21, 0, True), (64, 9, 1, False)])
def test_mid_size_sets_under_forced_join_tiers(seed, tier, tier0, protein):
    from pandelos_amd.calculate_k import calculate_k
    from pandelos_amd.synth import make_gene_set
    rng = np.random.default_rng(seed)
    gs = make_gene_set(genomes=int(rng.integers(6, 24)), genes_per_genome=int(rng.integers(150, 400)), mean_len=int(rng.integers(80, 200)),
                       sub_rate=0.1, seed=seed, protein_like=protein)
    k = calculate_k(gs.residues)
    base, query = _split(gs.residues, gs.offsets, gs.genome_of, int(gs.genome_of.max()))
    nat = _native(k, *base, options=[("join_tier1", tier), ("join_tier0", tier0)])
    nat.score_all()
    _check_against_oracle(nat, base, query, k, f"seed {seed} tier {tier}")
    nat.close()


def test_64_genome_protein_like_base_plus_one():
    from pandelos_amd.synth import make_gene_set
    gs = make_gene_set(genomes=65, genes_per_genome=750, mean_len=370, sub_rate=0.25, seed=6465, protein_like=True)
    base, query = _split(gs.residues, gs.offsets, gs.genome_of, 64)
    nat = _native(5, *base)
    _check_against_oracle(nat, base, query, 5, "64+1")
    nat.close()


def test_canonical_order():
    from pandelos_amd import _lib
    fx, base, query, k, G = load_case("protein_like_held_out")
    res_b, off_b, gen_b = base.flatten()
    nat = _native(k, res_b, off_b, gen_b, flags=_lib.PDL_FLAG_CANONICAL_ORDER)
    got = nat.query_idata(query).as_dict()
    order = np.lexsort((fx["column"], fx["row"]))
    for f in ("scores", "percs", "tr_percs", "row", "column"):
        assert np.array_equal(H.raw(got[f]), fx[f][order]), f
    for f in ("max_genome_score", "max_genome_score_col", "scoresMaxMappings"):
        assert np.array_equal(H.raw(got[f]), fx[f]), f
    nat.close()


def test_base_built_with_a_genome_shard():
    fx, base, query, k, G = load_case("protein_like_held_out")
    res_b, off_b, gen_b = base.flatten()
    nat = _native(k, res_b, off_b, gen_b, shard=[0, 2])
    assert_block(nat.query_idata(query).as_dict(), fx, "shard")
    nat.close()


def test_the_base_context_is_left_as_it_was():
    fx, base, query, k, G = load_case("protein_like_held_out")
    res_b, off_b, gen_b = base.flatten()
    nat = _native(k, res_b, off_b, gen_b)
    before = [nat.generate_scores_part(g).as_dict() for g in range(G)]
    edges = [nat.generate_edges_part(g) for g in range(G)]
    dic = nat.dictionary()
    costs = [nat.genome_cost(g) for g in range(G)]
    tm = nat.timings()
    a = nat.query_idata(query).as_dict()
    b = nat.query_idata(query).as_dict()
    H.assert_scores_equal(a, b, "two queries")
    for g in range(G):
        H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), before[g], f"base genome {g}")
        e = nat.generate_edges_part(g)
        assert all(np.array_equal(x, y) for x, y in zip(e, edges[g])), g
        assert nat.genome_cost(g) == costs[g]
    after = nat.dictionary()
    assert all(np.array_equal(x, y) for x, y in zip(after, dic))
    assert nat.timings() == tm
    # a rebuilt base (other data) answers its own queries, not the old one's
    nat.preprocess(k, res_b, off_b, gen_b)
    assert_block(nat.query_idata(query).as_dict(), fx, "after a second preprocess")
    nat.close()


def test_refusals():
    from pandelos_amd import _lib
    from pandelos_amd.pangene_native import PangeneNative
    fx, base, query, k, G = load_case("identical_gene")
    res_b, off_b, gen_b = base.flatten()
    rq, oq, _ = query.flatten()

    def code(fn):
        with pytest.raises(_lib.PdlError) as e:
            fn()
        return e.value.code, str(e.value)

    fresh = PangeneNative.open()
    assert code(lambda: fresh.query_scores(rq, oq))[0] == _lib.PDL_ERR_STATE
    fresh.close()
    cplx = PangeneNative.from_arrays(k, res_b, off_b, gen_b, only_complexity=True)
    assert code(lambda: cplx.query_scores(rq, oq))[0] == _lib.PDL_ERR_STATE
    cplx.close()
    low = PangeneNative.open()
    low.set_option("low_memory", 1)
    low.preprocess(k, res_b, off_b, gen_b)
    assert code(lambda: low.query_scores(rq, oq))[0] == _lib.PDL_ERR_STATE
    low.close()
    nat = _native(k, res_b, off_b, gen_b)
    assert code(lambda: nat.query_scores(rq, np.zeros(1, np.uint64)))[0] == _lib.PDL_ERR_ARGUMENT      # n_query == 0
    assert code(lambda: nat.query_scores(rq, np.array([0, 5, 3], np.uint64)))[0] == _lib.PDL_ERR_ARGUMENT
    c, msg = code(lambda: nat.query_scores(np.frombuffer(b"ACAZZ", np.uint8), np.array([0, 5], np.uint64)))
    assert c == _lib.PDL_ERR_UNSUPPORTED and "0x5a" in msg and "'Z'" in msg
    # NULL pointers through the C ABI itself
    import ctypes as C
    s = _lib.PdlScores()
    assert nat._lib.pdl_query_scores(nat._ctx, rq.ctypes.data, None, 1, C.byref(s), None) == _lib.PDL_ERR_ARGUMENT
    assert nat._lib.pdl_query_scores(nat._ctx, rq.ctypes.data, oq.ctypes.data, len(oq) - 1, None, None) == _lib.PDL_ERR_ARGUMENT
    from pandelos_amd.pangene_idata import PangeneIData
    with pytest.raises(ValueError):
        nat.query_idata(PangeneIData.from_arrays(rq, oq[:3], np.array([0, 1], np.uint32)))
    # still usable after the refusals
    assert_block(nat.query_idata(query).as_dict(), fx, "after refusals")
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
        nat.query_scores(rq, oq)
    assert e.value.code == _lib.PDL_ERR_STATE
    nat.close()


def test_query_command_end_to_end(tmp_path):
    from oracle import binding as ob
    from pandelos_amd import query as Q
    from pandelos_amd.pangenes import bbh_edges, net_lines
    from pandelos_amd.scores import Scores
    fx, base, query, k, G = load_case("protein_like_held_out")
    bf, qf, net, cells = tmp_path / "base.faa", tmp_path / "new.faa", tmp_path / "new.net", tmp_path / "new.tsv"
    bf.write_bytes(fx["base_faa"].tobytes())
    qf.write_bytes(fx["query_faa"].tobytes())
    assert Q.main(["-i", str(bf), "-k", str(k), "-q", str(qf), "-o", str(net), "--cells", str(cells)]) == 0
    res, off, gen, _ = union_arrays(base, query)
    want = ob.Oracle(res, off, gen, k).scores(G)
    s = Scores(scoresCount=int(want["scoresCount"]), **{f: np.asarray(want[f]) for f in H.FIELDS})
    assert net.read_text() == "".join(net_lines(*bbh_edges(s)))
    rows = cells.read_text().splitlines()
    assert len(rows) == int(want["scoresCount"])
    names = list(base.sequenceName) + list(query.sequenceName)
    first = rows[0].split("\t")
    assert first[0] == names[int(want["row"][0])] and first[1] == names[int(want["column"][0])]
    assert float(first[3]) == float(want["scores"][0])
