"""pdl_append_genomes on the GPU: a context grown by a merge must be, bit for bit, the context pdl_preprocess leaves on the
union — against the reference's digests and fixtures, a union build on the device and the CPU oracle; the corners of the merge;
the refusals, which leave the context alone; the append command end to end."""
import gzip
import json
import os

import numpy as np
import pytest

from tests import helpers as H
from tests.test_append_cpu import APPEND_SEED0, APPEND_SEEDS_DEFAULT
from tests.test_gpu_query import _native, _random_case, _split, _union
from tests.test_query_golden import CASES, assert_block, load_case

pytestmark = pytest.mark.gpu
N_SEEDS = int(os.environ.get("PDL_APPEND_SEEDS", str(APPEND_SEEDS_DEFAULT)))
BASE = json.loads((H.GOLDEN / "digests_baseline.json").read_text())


def _prefix(res, off, gen, genomes):
    """The first `genomes` genomes of a set whose genomes are laid out one after the other (make_gene_set)."""
    n = int((gen < genomes).sum())
    assert (gen[:n] < genomes).all()
    end = int(off[n])
    return res[:end], off[:n + 1], gen[:n]


def _genome(res, off, gen, lo, hi):
    """(residues, offsets from 0, genome ids) of the genes of genomes lo..hi-1 (consecutive genes)."""
    ids = np.nonzero((gen >= lo) & (gen < hi))[0]
    a, b = int(ids[0]), int(ids[-1]) + 1
    assert b - a == len(ids)
    o = off[a:b + 1].astype(np.uint64)
    return res[int(o[0]):int(o[-1])], o - o[0], gen[a:b]


def _assert_same_context(a, b, label, edges=True):
    """Every observable of context `a` equals that of context `b`."""
    assert a.cost.as_dict() == b.cost.as_dict(), label
    for x, y in zip(a.dictionary(), b.dictionary()):
        assert np.array_equal(x, y), f"{label}: dictionary"
    for x, y in zip(a.sequence_costs(), b.sequence_costs()):
        assert np.array_equal(x, y), f"{label}: sequence costs"
    ta, tb = a.rank_table(), b.rank_table()
    assert np.array_equal(ta[0], tb[0]) and ta[1] == tb[1], f"{label}: rank table"
    assert np.array_equal(a.scores_counts(), b.scores_counts()), f"{label}: score counts"
    for g in range(b.cost.genomes):
        assert a.genome_cost(g) == b.genome_cost(g), f"{label}: genome {g} cost"
        H.assert_scores_equal(a.generate_scores_part(g).as_dict(), b.generate_scores_part(g).as_dict(), f"{label} genome {g}")
        if edges:
            for x, y in zip(a.generate_edges_part(g), b.generate_edges_part(g)):
                assert np.array_equal(H.raw(x), H.raw(y)), f"{label}: edges of genome {g}"


def _assert_oracle(nat, res, off, gen, k, label, ora=None):
    from oracle import binding as ob
    ora = ora or ob.Oracle(res, off, gen, k)
    assert nat.cost.genomes == ora.genomes and nat.cost.total_cost == ora.total_cost, label
    for g in range(ora.genomes):
        H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), ora.scores(g), f"{label} genome {g} vs oracle")
        assert nat.genome_cost(g) == ora.genome_cost(g), f"{label} genome {g} cost"


def _append_vs_union(base, query, k, label, flags=0, options=(), oracle=True, edges=True, late=(), ora=None):
    """`late`: options set between the base's build and the append; the union is built under what is in force at the end."""
    res, off, gen, G = _union(base, query)
    nat = _native(k, *base, flags=flags, options=options, late=late)
    base_records = nat.cost.dictionary_records
    nat.append(*query)
    assert nat.cost.genomes == G + 1 and nat.cost.sequences == len(gen), label
    uni = _native(k, res, off, gen, flags=flags, options=tuple(options) + tuple(late))
    _assert_same_context(nat, uni, label, edges=edges)
    if oracle and not flags:
        _assert_oracle(nat, res, off, gen, k, label, ora=ora)
    info = nat.last_append_info
    assert info["residues"] == len(query[0]) and info["records"] == uni.cost.dictionary_records - base_records, label
    uni.close()
    return nat


# ---- 1. the reference's digests ----------------------------------------------------------------------------------------
def _check_digests(nat, d, label):
    assert nat.cost.total_cost == d["total_cost"], label
    assert [nat.genome_cost(g) for g in range(d["genomes"])] == d["genome_cost"], label
    H.assert_scores_match_digest(lambda g: nat.generate_scores_part(g).as_dict(), d, label)


@pytest.mark.parametrize("name", ["salmonella7_standin", "mycoplasma64_standin"])
def test_last_genome_appended_matches_the_reference_digests(name):
    from pandelos_amd.pangene_native import PangeneNative
    d = BASE[name]
    gs = H.make_gene_set(**d["shape"])
    res, off, gen, k, G = gs.residues, gs.offsets, gs.genome_of, d["k"], d["genomes"]
    nat = PangeneNative.from_arrays(k, *_prefix(res, off, gen, G - 1))
    nat.append(*_genome(res, off, gen, G - 1, G)[:2])
    assert nat.cost.sequences == d["sequences"] and nat.cost.genomes == G
    _check_digests(nat, d, f"{name}: {G - 1} + 1")
    nat.close()


def test_four_genomes_appended_one_by_one_and_at_once_match_the_reference_digests():
    from pandelos_amd.pangene_native import PangeneNative
    name = "mycoplasma64_standin"
    d = BASE[name]
    gs = H.make_gene_set(**d["shape"])
    res, off, gen, k = gs.residues, gs.offsets, gs.genome_of, d["k"]
    one = PangeneNative.from_arrays(k, *_prefix(res, off, gen, 60))
    for g in range(60, 64):
        one.append(*_genome(res, off, gen, g, g + 1)[:2])
        assert one.cost.genomes == g + 1
    _check_digests(one, d, "60 + 1 + 1 + 1 + 1")
    four = PangeneNative.from_arrays(k, *_prefix(res, off, gen, 60))
    four.append(*_genome(res, off, gen, 60, 64))
    _check_digests(four, d, "60 + 4")
    _assert_same_context(one, four, "one by one vs at once")
    one.close(); four.close()


# ---- 2. the same context as a union build ------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,tier,tier0,protein", [(61, 10, 0, False), (62, 11, 1, True), (63, 21, 0, True), (64, 9, 1, False)])
def test_mid_size_sets_equal_a_union_build(seed, tier, tier0, protein):
    from pandelos_amd.calculate_k import calculate_k
    from pandelos_amd.synth import make_gene_set
    rng = np.random.default_rng(seed)
    gs = make_gene_set(genomes=int(rng.integers(6, 24)), genes_per_genome=int(rng.integers(150, 400)), mean_len=int(rng.integers(80, 200)),
                       sub_rate=0.1, seed=seed, protein_like=protein)
    k = calculate_k(gs.residues)
    base, query = _split(gs.residues, gs.offsets, gs.genome_of, int(gs.genome_of.max()))
    _append_vs_union(base, query, k, f"seed {seed} tier {tier}", options=[("join_tier1", tier), ("join_tier0", tier0)]).close()


def test_64_genome_protein_like_base_plus_one_equals_a_union_build():
    from pandelos_amd.synth import make_gene_set
    gs = make_gene_set(genomes=65, genes_per_genome=750, mean_len=370, sub_rate=0.25, seed=6465, protein_like=True)
    base, query = _split(gs.residues, gs.offsets, gs.genome_of, 64)
    _append_vs_union(base, query, 5, "64+1").close()


# ---- 3. query after append, append after query; the reference-pinned query fixtures ------------------------------------------
def test_query_then_append_then_query_then_append():
    from oracle import binding as ob
    from pandelos_amd.synth import make_gene_set
    gs = make_gene_set(genomes=7, genes_per_genome=90, mean_len=110, sub_rate=0.12, seed=8123, protein_like=True)
    res, off, gen, k = gs.residues, gs.offsets, gs.genome_of, 4
    base = _prefix(res, off, gen, 5)
    A, B = _genome(res, off, gen, 5, 6)[:2], _genome(res, off, gen, 6, 7)[:2]
    upto6 = _prefix(res, off, gen, 6)
    nat = _native(k, *base)
    H.assert_scores_equal(nat.query_scores(*A).as_dict(), ob.Oracle(*upto6, k).scores(5), "query A")
    nat.append(*A)
    _assert_oracle(nat, *upto6, k, "base + A")
    ora = ob.Oracle(res, off, gen, k)
    H.assert_scores_equal(nat.query_scores(*B).as_dict(), ora.scores(6), "query B on base + A")
    assert nat.last_query_info["genome_cost"] == ora.genome_cost(6)
    nat.append(*B)
    _assert_oracle(nat, res, off, gen, k, "base + A + B")
    nat.close()


@pytest.mark.parametrize("name", CASES)
def test_appended_query_fixture_gives_the_fixture_block(name):
    from pandelos_amd.pangene_native import PangeneNative
    fx, base, query, k, G = load_case(name)
    nat = PangeneNative(k, base)
    nat.append_idata(query)
    assert nat.cost.genomes == G + 1
    assert_block(nat.generate_scores_part(G).as_dict(), fx, name)
    assert nat.genome_cost(G) == int(fx["genome_cost"])
    nat.close()


# ---- 4. random small sets ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", list(range(APPEND_SEED0, APPEND_SEED0 + N_SEEDS)))
def test_random_small_sets_equal_a_union_build_and_the_oracle(seed):
    case = _random_case(seed)
    if case is None:
        pytest.skip("seed gives no usable split")
    base, query, k = case
    _append_vs_union(base, query, k, f"seed {seed}", edges=False).close()


# ---- 5. the corners the merge can get wrong ----------------------------------------------------------------------------------
@pytest.mark.parametrize("letters,k", [(22, 15), (24, 14)])
def test_wrapped_keys_merge_in_the_order_of_the_sorted_bytes(letters, k):
    """B^k passes 2^64 unnoticed: the ranks fill 64 bits while rank_init counts fewer, and the stream is ordered by the bytes
    the sort's passes cover."""
    gs = H.wrapped_rank_set(letters, seed=letters * 100 + k)
    base, query = _split(gs.residues, gs.offsets, gs.genome_of, int(gs.genome_of.max()))
    nat = _append_vs_union(base, query, k, f"{letters} letters, k = {k}")
    assert nat.cost.hash_fallback == 0 and nat.cost.rank_bits < 64
    nat.close()


@pytest.mark.parametrize("case", ["synth_5x60x80_k13", "synth_5x60x80_k14"])
def test_64_bit_keys_without_hashing(case):
    res, off, gen, k, _ = H.load_small(case)
    base, query = _split(res, off, gen, int(gen.max()))
    nat = _append_vs_union(base, query, k, case)
    assert nat.cost.rank_bits > 32 and nat.cost.hash_fallback == 0
    nat.close()


def _pack(seqs, genome_of):
    res = np.frombuffer(b"".join(seqs), np.uint8).copy()
    off = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(x) for x in seqs], out=off[1:])
    return res, off, np.asarray(genome_of, np.uint32)


@pytest.mark.parametrize("letter", [b"A", b"Y"])
def test_newcomers_below_and_above_every_base_kmer(letter):
    """A base of letters in between plus one poly-A and one poly-Y gene (so both letters are in the alphabet); the newcomer's
    genes are all poly-A / all poly-Y: every new k-mer ties with the smallest / largest base k-mer, the tiles hold the new
    elements at one end."""
    rng = np.random.default_rng(11)
    mid = np.frombuffer(b"CDEFGHIKLMNPQRSTVW", np.uint8)
    seqs = [b"A" * 40, b"Y" * 40] + [mid[rng.integers(0, len(mid), int(rng.integers(60, 160)))].tobytes() for _ in range(120)]
    base = _pack(seqs, [min(i // 41, 2) for i in range(len(seqs))])
    new = _pack([letter * int(n) for n in (300, 7, 2600, 4, 90)], [0] * 5)[:2]
    _append_vs_union(base, new, 4, f"poly-{letter.decode()}").close()


def test_a_newcomer_identical_to_a_base_genome():
    from pandelos_amd.synth import make_gene_set
    gs = make_gene_set(genomes=4, genes_per_genome=200, mean_len=120, sub_rate=0.1, seed=515)
    base = (gs.residues, gs.offsets, gs.genome_of)
    twin = _genome(gs.residues, gs.offsets, gs.genome_of, 2, 3)[:2]
    _append_vs_union(base, twin, 4, "twin of genome 2").close()


def test_a_newcomer_without_any_kmer():
    from pandelos_amd.synth import make_gene_set
    gs = make_gene_set(genomes=4, genes_per_genome=30, mean_len=60, sub_rate=0.1, seed=77)
    base = (gs.residues, gs.offsets, gs.genome_of)
    new = (gs.residues[:3].copy(), np.array([0, 0, 2, 3], np.uint64))           # an empty gene, two genes shorter than k
    nat = _append_vs_union(base, new, 3, "no k-mer")
    assert nat.cost.sequences == gs.genes + 3 and nat.cost.genomes == 5 and nat.last_append_info["kmer_occurrences"] == 0
    assert nat.generate_scores_part(4).scoresCount == 0
    nat.close()


def test_base_built_from_device_input_that_is_freed_before_the_append():
    import torch
    from pandelos_amd.pangene_native import PangeneNative
    from pandelos_amd.synth import make_gene_set
    gs = make_gene_set(genomes=6, genes_per_genome=150, mean_len=100, sub_rate=0.1, seed=909)
    base, query = _split(gs.residues, gs.offsets, gs.genome_of, 5)
    rb, ob_, gb = base
    dev = torch.device("cuda", 0)
    t_res = torch.from_numpy(np.concatenate([rb, np.zeros(32, np.uint8)])).to(dev)
    t_off = torch.from_numpy(ob_.astype(np.int64)).to(dev)
    t_gen = torch.from_numpy(gb.astype(np.int32)).to(dev)
    nat = PangeneNative.from_device(4, t_res.data_ptr(), t_off.data_ptr(), t_gen.data_ptr(), len(gb), len(rb))
    torch.cuda.synchronize()
    t_res.fill_(0); t_off.fill_(0); t_gen.fill_(0x7fffffff)       # whoever still read the caller's buffers would notice
    torch.cuda.synchronize()
    del t_res, t_off, t_gen
    torch.cuda.empty_cache()
    nat.append(*query)
    res, off, gen, _ = _union(base, query)
    uni = _native(4, res, off, gen)
    _assert_same_context(nat, uni, "device input")
    nat.close(); uni.close()


def test_canonical_order_flag():
    from pandelos_amd import _lib
    fx, base, query, k, G = load_case("protein_like_held_out")
    b, q = base.flatten(), query.flatten()[:2]
    _append_vs_union(b, q, k, "canonical order", flags=_lib.PDL_FLAG_CANONICAL_ORDER).close()


def test_append_info_and_timings_describe_the_append():
    from pandelos_amd.pangene_native import PangeneNative
    d = BASE["salmonella7_standin"]
    gs = H.make_gene_set(**d["shape"])
    res, off, gen = gs.residues, gs.offsets, gs.genome_of
    nat = PangeneNative.from_arrays(d["k"], *_prefix(res, off, gen, 6))
    nat.score_all()
    new = _genome(res, off, gen, 6, 7)
    nat.append(*new[:2])
    info, tm = nat.last_append_info, nat.timings()
    m = int(np.maximum(np.diff(new[1].astype(np.int64)) - d["k"] + 1, 0).sum())
    assert info["kmer_occurrences"] == m and info["residues"] == len(new[0]) and 0 < info["records"] <= m
    assert info["rank_sort_ms"] > 0 and info["merge_ms"] > 0 and info["device_ms"] >= info["rank_sort_ms"] + info["merge_ms"]
    assert tm["preprocess_total_ms"] == info["device_ms"] and tm["hist_ms"] == 0 and tm["join_ms"] == 0 and tm["emitted_cells"] == 0
    assert abs(tm["sort_rank_ms"] + tm["rank_ms"] - info["rank_sort_ms"] - info["merge_ms"]) < 1e-3
    nat.close()


# ---- 6. refusals leave the context alone ---------------------------------------------------------------------------------------
def _snapshot(nat):
    G = nat.cost.genomes
    return ([nat.generate_scores_part(g).as_dict() for g in range(G)], [nat.generate_edges_part(g) for g in range(G)], nat.dictionary(),
            [nat.genome_cost(g) for g in range(G)], nat.sequence_costs(), nat.cost.as_dict(), nat.timings())


def _assert_snapshot(nat, snap, label):
    scores, edges, dic, costs, seqc, cost, tm = snap
    assert nat.cost.as_dict() == cost, label
    for g in range(len(scores)):
        H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), scores[g], f"{label} genome {g}")
        assert all(np.array_equal(x, y) for x, y in zip(nat.generate_edges_part(g), edges[g])), f"{label} edges {g}"
        assert nat.genome_cost(g) == costs[g], label
    assert all(np.array_equal(x, y) for x, y in zip(nat.dictionary(), dic)), label
    assert all(np.array_equal(x, y) for x, y in zip(nat.sequence_costs(), seqc)), label
    if tm is not None:
        assert nat.timings() == tm, label


def test_refusals_leave_the_context_as_it_was():
    import ctypes as C
    from pandelos_amd import _lib
    from pandelos_amd.pangene_native import PangeneNative
    fx, base, query, k, G = load_case("protein_like_held_out")
    res_b, off_b, gen_b = base.flatten()
    rq, oq, _ = query.flatten()
    n = len(oq) - 1

    def code(fn):
        with pytest.raises(_lib.PdlError) as e:
            fn()
        return e.value.code, str(e.value)

    fresh = PangeneNative.open()
    assert code(lambda: fresh.append(rq, oq))[0] == _lib.PDL_ERR_STATE
    fresh.close()
    cplx = PangeneNative.from_arrays(k, res_b, off_b, gen_b, only_complexity=True)
    assert code(lambda: cplx.append(rq, oq))[0] == _lib.PDL_ERR_STATE
    assert cplx.cost.genomes == G
    cplx.close()
    low = PangeneNative.open()
    low.set_option("low_memory", 1)
    low.preprocess(k, res_b, off_b, gen_b)
    assert code(lambda: low.append(rq, oq))[0] == _lib.PDL_ERR_STATE
    low.close()
    shard = _native(k, res_b, off_b, gen_b, shard=[0, 2])
    before = shard.generate_scores_part(2).as_dict()
    assert code(lambda: shard.append(rq, oq))[0] == _lib.PDL_ERR_STATE
    H.assert_scores_equal(shard.generate_scores_part(2).as_dict(), before, "shard")
    shard.close()

    nat = _native(k, res_b, off_b, gen_b)
    snap = _snapshot(nat)
    assert code(lambda: nat.append(rq, np.zeros(1, np.uint64)))[0] == _lib.PDL_ERR_ARGUMENT            # n == 0
    assert code(lambda: nat.append(rq, np.array([0, 5, 3], np.uint64)))[0] == _lib.PDL_ERR_ARGUMENT     # offsets decrease
    assert code(lambda: nat.append(rq, oq, np.full(n, G - 1, np.uint32)))[0] == _lib.PDL_ERR_ARGUMENT   # joins an existing genome
    assert code(lambda: nat.append(rq, oq, np.full(n, G + 1, np.uint32)))[0] == _lib.PDL_ERR_ARGUMENT   # skips id G
    if n >= 3:
        ids = np.full(n, G, np.uint32); ids[1] = G + 1; ids[2] = G + 3
        assert code(lambda: nat.append(rq, oq, ids))[0] == _lib.PDL_ERR_ARGUMENT                         # not dense
    info = _lib.PdlAppendInfo()
    assert nat._lib.pdl_append_genomes(nat._ctx, rq.ctypes.data, None, None, 1, None, C.byref(info)) == _lib.PDL_ERR_ARGUMENT
    assert nat._lib.pdl_append_genomes(nat._ctx, None, oq.ctypes.data, None, n, None, None) == _lib.PDL_ERR_ARGUMENT
    assert nat._lib.pdl_append_genomes(None, rq.ctypes.data, oq.ctypes.data, None, n, None, None) == _lib.PDL_ERR_ARGUMENT
    c, msg = code(lambda: nat.append(np.frombuffer(b"ACAZZ", np.uint8), np.array([0, 5], np.uint64)))
    assert c == _lib.PDL_ERR_UNSUPPORTED and "0x5a" in msg and "'Z'" in msg
    _assert_snapshot(nat, snap, "after the refusals")
    # ... and it still takes the append, and a preprocess afterwards behaves as on a fresh context
    nat.append(rq, oq)
    assert_block(nat.generate_scores_part(G).as_dict(), fx, "append after the refusals")
    nat.preprocess(k, res_b, off_b, gen_b)
    _assert_snapshot(nat, snap[:-1] + (None,), "preprocess after an append")          # (its timings are those of the new build)
    assert_block(nat.query_idata(query).as_dict(), fx, "query after that")
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
        nat.append(rq, oq)
    assert e.value.code == _lib.PDL_ERR_STATE
    nat.close()


# ---- 7. end to end -------------------------------------------------------------------------------------------------------
def _write_faa(gs, path, lo, hi):
    res = gs.residues.tobytes()
    with open(path, "wb") as f:
        for i in np.nonzero((gs.genome_of >= lo) & (gs.genome_of < hi))[0]:
            g = int(gs.genome_of[i])
            f.write(b"G%d\tg%d_%d@G%d:1\tprod %d\n" % (g, g, i, g, int(gs.family_of[i])))
            f.write(res[int(gs.offsets[i]):int(gs.offsets[i + 1])])
            f.write(b"\n")


def test_append_command_writes_the_canonical_net(tmp_path):
    from pandelos_amd import append as A
    name = "mycoplasma64_standin"
    gs = H.make_gene_set(**BASE[name]["shape"])
    base, n1, n2, net = tmp_path / "base.faa", tmp_path / "n1.faa", tmp_path / "n2.faa", tmp_path / "union.net"
    _write_faa(gs, base, 0, 62); _write_faa(gs, n1, 62, 63); _write_faa(gs, n2, 63, 64)
    assert A.main(["-i", str(base), "-k", str(BASE[name]["k"]), "-a", str(n1), "-a", str(n2), "-o", str(net)]) == 0
    want = gzip.open(H.GOLDEN / "net" / f"{name}.net.gz", "rb").read()
    assert net.read_bytes() == want
