"""Option "query_rekey" on the GPU: pdl_query_scores, pdl_query_batch, pdl_place_query and pdl_place_batch for queries that bring
letters the base lacks (pandelos_amd/csrc/pdl_query.h, pdl_query_batch.h, pdl_rekey.h: Q-rebase).

  * the reference-pinned fixtures of tests/golden/query_rekey, bit for bit, with the genome cost;
  * single queries against the CPU oracle on the union at forced key widths, record counts and the HBM join;
  * the block against compute_scores(G) of a context the same genes were appended to under "alphabet_rekey", the placement's
    edges against its compute_edges(G), the placement against the numpy contract;
  * batches: every block and placement equals the single call's under the default chunking and in chunks of one; a chunk whose
    joint alphabet is inexact is cut and still answers;
  * refusals (a union that wraps, a hashed base) leave `out` zeroed and the context as it was; with the option off the words stay;
  * state and pdl_get_query_rekey_info; random seeds of tests/query_rekey_sets.py, none skipped."""
import ctypes as C
import os

import numpy as np
import pytest

from pandelos_amd import _lib
from pandelos_amd import place as P
from tests import helpers as H
from tests import query_rekey_sets as S
from tests.test_gpu_place import _base_edges
from tests.test_gpu_query import _genes, _native, _union
from tests.test_gpu_query_batch import _assert_snapshot, _snapshot
from tests.test_place_cpu import assert_placement
from tests.test_query_golden import assert_block
from tests.test_query_golden import load_case as load_plain_case
from tests.test_rekey_cpu import family_genes, pack, with_letters

pytestmark = pytest.mark.gpu
N_SEEDS = int(os.environ.get("PDL_QUERY_REKEY_SEEDS", str(S.SEEDS_DEFAULT)))
REKEY = (("query_rekey", 1),)
A18, A20 = b"ACDEFGHIKLMNPQRSTV", b"ACDEFGHIKLMNPQRSTVWY"


def _check_against_oracle(nat, base, query, k, label):
    from oracle import binding as ob
    res, off, gen, G = _union(base, query)
    ora = ob.Oracle(res, off, gen, k)
    got = nat.query_scores(*query).as_dict()
    H.assert_scores_equal(got, ora.scores(G), label)
    assert nat.last_query_info["genome_cost"] == ora.genome_cost(G), label
    return got


def _family_case(alphabet, add, k, seed, genes=6, lo=None, hi=None, genomes=3):
    """-> (base arrays, query (res, off)): `genomes` base genomes over `alphabet`, the query their sibling with `add` sprinkled in"""
    lo, hi = lo or k + 2, hi or k + 40
    fam = family_genes(alphabet, genomes + 1, genes, lo, hi, seed)
    fam[0][0] = bytes(alphabet) + fam[0][0]
    base = pack([g for gs in fam[:genomes] for g in gs], [i for i, gs in enumerate(fam[:genomes]) for _ in gs])
    q = [with_letters(g, add, seed + j) if add else g for j, g in enumerate(fam[genomes])]
    res, off, _ = pack(q, [0] * len(q))
    return base, (res, off)


def _code(fn):
    with pytest.raises(_lib.PdlError) as e:
        fn()
    return e.value.code, str(e.value)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.CASES)
def test_fixture(name):
    fx, base, query, k, G = S.load_case(name)
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative(k, base)
    c, msg = _code(lambda: nat.query_idata(query))
    assert c == _lib.PDL_ERR_UNSUPPORTED and "the union would rank k-mers differently" in msg      # (the option is off)
    nat.set_option("query_rekey", 1)
    got = nat.query_idata(query).as_dict()
    assert_block(got, fx, name)
    info = nat.last_query_info
    assert info["genome_cost"] == int(fx["genome_cost"])
    assert info["kmer_occurrences"] >= info["records"] >= info["matched_records"]
    rk = nat.last_query_rekey_info
    assert rk["queries_rekeyed"] == 1 and rk["records_rebased"] == info["records"] and rk["letters_max"] > rk["letters_base"]
    nat.close()


# ---- single queries against the oracle on the union ----------------------------------------------------------------------------------
@pytest.mark.parametrize("alphabet,add,k,bits", [(b"ACGT", b"N", 16, (32, 38)), (b"AC", b"G", 32, (32, 51)), (b"ACGT", b"N", 27, (54, 63)),
                                                 (A20, b"X", 8, (35, 36)), (b"CDEF", b"*", 5, (10, 12))],
                         ids=["ACGT+N_k16", "AC+G_k32", "ACGT+N_k27", "20+X_k8", "CDEF+star_k5"])
def test_key_widths(alphabet, add, k, bits):
    base, query = _family_case(alphabet, add, k, 100 + k)
    nat = _native(k, *base, options=REKEY)
    _check_against_oracle(nat, base, query, k, f"{alphabet} + {add} at k = {k}")
    rk = nat.last_query_rekey_info
    assert (rk["key_bits_base"], rk["key_bits_max"]) == bits and rk["letters_base"] == len(alphabet) and rk["letters_max"] == len(alphabet) + len(add)
    nat.close()


def _distinct_kmer_gene(records, k, seed):
    """a gene over 20 letters with exactly `records` k-mers, all different, one of them (or, of one: it) holding an 'X'"""
    letters = np.frombuffer(A20, np.uint8)
    while True:
        g = letters[np.random.default_rng(seed).integers(0, 20, records + k - 1)].tobytes()
        g = g[:k // 2] + b"X" + g[k // 2 + 1:]
        if len({g[i:i + k] for i in range(records)}) == records:
            return g
        seed += 1000


@pytest.mark.parametrize("records", [1, 255, 256, 257, 258])
def test_record_counts_around_a_workgroup(records):
    k = 4
    base, _ = _family_case(A20, b"X", k, 7, genes=8, lo=60, hi=120)
    gene = _distinct_kmer_gene(records, k, records)
    nat = _native(k, *base, options=REKEY)
    _check_against_oracle(nat, base, _genes(gene), k, f"{records} records")
    assert nat.last_query_info["records"] == records and nat.last_query_rekey_info["records_rebased"] == records
    nat.close()


def test_a_query_without_a_kmer_that_brings_a_letter_in_a_short_gene():
    k = 4
    base, _ = _family_case(A20, b"X", k, 9)
    nat = _native(k, *base, options=REKEY)
    got = _check_against_oracle(nat, base, _genes(b"AX", b"C", b""), k, "no k-mer")
    assert got["scoresCount"] == 0 and nat.last_query_info["records"] == 0
    rk = nat.last_query_rekey_info
    assert rk["queries_rekeyed"] == 1 and rk["records_rebased"] == 0 and rk["letters_max"] == 21
    _check_against_oracle(nat, base, _genes(b"ACDEFGH"), k, "a plain query behind it")
    assert nat.last_query_rekey_info["queries_rekeyed"] == 0
    nat.close()


def test_wide_row_with_a_new_letter_reaches_the_hbm_join():
    fx, base, query, k, G = load_plain_case("wide_row_9000_columns")
    b = base.flatten()
    nat = _native(k, *b, options=REKEY)
    got = _check_against_oracle(nat, b, _genes(b"AAAA", b"CXEFAAA"), k, "wide row, one residue replaced by X")
    assert int((np.asarray(got["row"]) == np.asarray(got["row"])[0]).sum()) > 8192
    assert_block(nat.query_idata(query).as_dict(), fx, "the plain wide row behind it")
    nat.close()


# ---- equivalences -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alphabet,add,k", [(b"CDEFGHIK", b"A", 3), (b"CDEFHIKL", b"GZ", 4), (b"ACGT", b"N", 16)], ids=["below", "two", "wider_keys"])
def test_block_edges_and_placement_equal_the_appended_contexts(alphabet, add, k):
    base, query = _family_case(alphabet, add, k, 300 + k, genes=8)
    res_b, off_b, gen_b = base
    N, n, G = len(gen_b), len(query[1]) - 1, int(gen_b.max()) + 1
    nat = _native(k, *base, options=REKEY)
    block = nat.query_scores(*query).as_dict()
    pl = nat.place_query(*query)
    union = _native(k, *base, options=(("alphabet_rekey", 1),))
    union.append(*query)
    assert union.last_rekey_info["rekeyed"] == 1
    H.assert_scores_equal(block, union.generate_scores_part(G).as_dict(), "block against the appended context")
    us, ud, usc = union.generate_edges_part(G)
    assert np.array_equal(pl["src"], us) and np.array_equal(pl["dst"], ud) and H.raw(pl["score"]).tobytes() == H.raw(usc).tobytes()
    union.close()
    bs, bd = _base_edges(nat, G)
    assert_placement(pl, P.placement_from_edges(bs, bd, gen_b, n, pl["src"], pl["dst"]), "placement")
    assert nat.last_place_info["query"]["genome_cost"] == nat.last_query_info["genome_cost"]
    nat.close()


# ---- batches ------------------------------------------------------------------------------------------------------------------------------
def _batch_queries(alphabet, k, seed):
    """six queries over one base: two plain, two with different new letters, one with two letters, one whose only new letter is in a
    gene shorter than k"""
    base, plain = _family_case(alphabet, b"", k, seed)
    fam = family_genes(alphabet, 6, 5, k + 2, k + 30, seed + 1)
    qs = []
    for j, add in enumerate((b"", b"X", b"", b"*", b"XZ", None)):
        genes = [with_letters(g, add, seed + 10 * j + i) if add else g for i, g in enumerate(fam[j])]
        if add is None:
            genes.insert(2, b"U" * (k - 1))
        res, off, _ = pack(genes, [0] * len(genes))
        qs.append((res, off))
    return base, qs


@pytest.mark.parametrize("chunk_bytes", [None, 1], ids=["default_chunks", "chunks_of_one"])
def test_batch_blocks_and_placements_equal_the_single_calls(chunk_bytes):
    k = 4
    base, qs = _batch_queries(b"CDEFGHIKLM", k, 41)
    nat = _native(k, *base, options=REKEY)
    singles = [nat.query_scores(*q).as_dict() for q in qs]
    costs = []
    for q in qs:
        nat.query_scores(*q)
        costs.append(nat.last_query_info["genome_cost"])
    places = [nat.place_query(*q) for q in qs]
    if chunk_bytes:
        nat.set_option("query_batch_bytes", chunk_bytes)
    blocks = nat.query_batch(qs)
    info = nat.last_query_batch_info
    assert info["chunks"] == (len(qs) if chunk_bytes else 1)
    for j, b in enumerate(blocks):
        H.assert_scores_equal(b.as_dict(), singles[j], f"query {j}")
        assert info["queries"][j]["genome_cost"] == costs[j], j
    rk = nat.last_query_rekey_info
    assert rk["queries_rekeyed"] == 4 and rk["letters_base"] == 10 and rk["letters_max"] == 12
    got = nat.place_batch(qs)
    for j, pl in enumerate(got):
        assert_placement(pl, places[j], f"placement {j}")
        assert np.array_equal(pl["src"], places[j]["src"]) and np.array_equal(pl["dst"], places[j]["dst"]), j
        assert H.raw(pl["score"]).tobytes() == H.raw(places[j]["score"]).tobytes(), j
    assert nat.last_query_rekey_info["queries_rekeyed"] == 4
    nat.close()


def _a18_case(k=15):
    assert 19 ** k < 1 << 64 <= 20 ** k                              # 18 letters + one: exact; + two: not
    fam = family_genes(A18, 3, 3, k + 2, k + 12, 77)
    fam[0][0] = A18 + fam[0][0]
    base = pack([g for gs in fam[:2] for g in gs], [i for i, gs in enumerate(fam[:2]) for _ in gs])
    w = _genes(*[with_letters(g, b"W", 5 + i) for i, g in enumerate(fam[2])])
    y = _genes(*[with_letters(g, b"Y", 9 + i) for i, g in enumerate(fam[2])])
    wy = _genes(*[with_letters(g, b"WY", 13 + i, every=5) for i, g in enumerate(fam[2])])
    assert {87, 89} <= set(wy[0].tolist())
    return base, w, y, wy


def test_a_chunk_whose_joint_alphabet_is_inexact_is_cut_and_still_answers():
    k = 15
    base, w, y, _ = _a18_case(k)
    plain = _genes(base[0][:int(base[1][1])].tobytes())
    nat = _native(k, *base, options=REKEY)
    singles = [_check_against_oracle(nat, base, q, k, "single") for q in (w, plain, y)]
    blocks = nat.query_batch([w, plain, y])
    for j, b in enumerate(blocks):
        H.assert_scores_equal(b.as_dict(), singles[j], f"query {j}")
    assert nat.last_query_batch_info["chunks"] == 2                  # cut in front of the query that brings the 20th letter
    rk = nat.last_query_rekey_info
    assert rk["queries_rekeyed"] == 2 and rk["letters_max"] == 19 and rk["key_bits_max"] == 64
    pls = nat.place_batch([w, plain, y])
    for j, q in enumerate((w, plain, y)):
        assert_placement(pls[j], nat.place_query(*q), f"placement {j}")
    nat.close()


def _cpu_chunks(base_res, queries, k):
    """the cut rule of a chunk on the CPU (rk_query's: base letters + the chunk's joint new letters must keep B^k below 2^64; a
    query that would tip that over starts the next chunk): -> the lists of query indices"""
    have = set(base_res.tolist())
    chunks, joint = [], set()
    for j, (res, _) in enumerate(queries):
        own = set(res.tolist()) - have
        if chunks and (own <= joint or (len(have) + len(joint | own)) ** k < 1 << 64):
            chunks[-1].append(j)
            joint |= own
        else:
            chunks.append([j])
            joint = set(own)
    return chunks


def test_a_chunk_cut_at_every_tipping_query_is_staged_once_and_read_as_prefixes():
    k = 15
    base, w, y, _ = _a18_case(k)
    plain = _genes(base[0][:int(base[1][1])].tobytes())
    short = _genes(b"AY", b"")                                       # no k-mer; its Y counts all the same
    qs = [w, y, short, w, plain, y]
    assert _cpu_chunks(base[0], qs, k) == [[0], [1, 2], [3, 4], [5]]
    nat = _native(k, *base, options=REKEY)
    singles, costs = [], []
    for q in qs:
        singles.append(nat.query_scores(*q).as_dict())
        costs.append(nat.last_query_info["genome_cost"])
    places = [nat.place_query(*q) for q in qs]
    blocks = nat.query_batch(qs)                                     # (default query_batch_bytes: only the alphabet cuts)
    info = nat.last_query_batch_info
    assert info["chunks"] == 4
    for j, b in enumerate(blocks):
        H.assert_scores_equal(b.as_dict(), singles[j], f"query {j}")
        assert info["queries"][j]["genome_cost"] == costs[j], j
    assert blocks[2].as_dict()["scoresCount"] == 0
    for j, pl in enumerate(nat.place_batch(qs)):
        assert_placement(pl, places[j], f"placement {j}")
    nat.set_option("query_rekey", 0)
    c, msg = _code(lambda: nat.query_batch(qs))
    assert c == _lib.PDL_ERR_UNSUPPORTED and "the union would rank k-mers differently" in msg and "query 0:" in msg, msg
    nat.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _raw_query(nat, q):
    """pdl_query_scores through ctypes with a stale `out`: -> (code, message); a refusal must leave `out` zeroed"""
    res, off = q
    s, info = _lib.PdlScores(), _lib.PdlQueryInfo()
    s.scoresCount, s.rows = 77, 88
    rc = nat._lib.pdl_query_scores(nat._ctx, res.ctypes.data, off.ctypes.data, len(off) - 1, C.byref(s), C.byref(info))
    if rc != _lib.PDL_OK:
        assert bytes(s) == bytes(C.sizeof(_lib.PdlScores)), "out is not zeroed after a refusal"
    else:
        nat._lib.pdl_free_scores(C.byref(s))
    return rc, nat._lib.pdl_last_error(nat._ctx).decode()


def test_a_union_that_would_wrap_is_refused_and_names_the_unions_side():
    k = 15
    base, w, y, wy = _a18_case(k)
    G = int(base[2].max()) + 1
    nat = _native(k, *base, options=REKEY)
    before = _snapshot(nat, G)
    info_before = nat.last_query_rekey_info
    rc, msg = _raw_query(nat, wy)
    assert rc == _lib.PDL_ERR_UNSUPPORTED and "union" in msg and "wrapped past 2^64" in msg and "query_rekey" in msg and "0x57" in msg, msg
    c, msg = _code(lambda: nat.query_batch([w, wy, y]))
    assert c == _lib.PDL_ERR_UNSUPPORTED and "query 1:" in msg and "union" in msg, msg
    c, msg = _code(lambda: nat.place_query(*wy))
    assert c == _lib.PDL_ERR_UNSUPPORTED and "union" in msg, msg
    c, msg = _code(lambda: nat.place_batch([w, wy]))
    assert c == _lib.PDL_ERR_UNSUPPORTED and "query 1:" in msg, msg
    assert nat.last_query_rekey_info == info_before                  # (the report is of the last SUCCESSFUL call)
    _assert_snapshot(nat, G, before, "after the refusals")
    _check_against_oracle(nat, base, w, k, "a legal query behind the refusals")
    nat.set_option("query_rekey", 0)
    c, msg = _code(lambda: nat.query_scores(*w))
    assert c == _lib.PDL_ERR_UNSUPPORTED and "query byte 0x57 ('W') is not in the base's alphabet: the union would rank k-mers differently" in msg, msg
    nat.close()


def test_a_hashed_base_is_refused_and_names_the_bases_side():
    fx, base, query, k, G = load_plain_case("hash_fallback_20_letters_k16")
    b = base.flatten()
    rq, oq, _ = query.flatten()
    rx = rq.copy()
    rx[3] = ord("X")
    nat = _native(k, *b, options=REKEY)
    before = _snapshot(nat, G)
    rc, msg = _raw_query(nat, (rx, oq))
    assert rc == _lib.PDL_ERR_UNSUPPORTED and "base's ranks are hashed" in msg and "query_rekey" in msg and "'X'" in msg, msg
    c, msg = _code(lambda: nat.query_batch([(rq, oq), (rx, oq)]))
    assert c == _lib.PDL_ERR_UNSUPPORTED and "query 1:" in msg and "base's ranks are hashed" in msg, msg
    _assert_snapshot(nat, G, before, "after the refusals")
    assert_block(nat.query_scores(rq, oq).as_dict(), fx, "a legal query behind the refusals")
    nat.close()


# ---- state --------------------------------------------------------------------------------------------------------------------------------
def test_rekeyed_and_plain_queries_in_turn_and_the_report():
    k = 16
    base, query = _family_case(b"ACGT", b"N", k, 55)
    _, other = _family_case(b"ACGT", b"NR", k, 56)
    plain = _genes(base[0][:int(base[1][2])].tobytes())
    G = int(base[2].max()) + 1
    nat = _native(k, *base, options=REKEY + (("alphabet_rekey", 1),))
    before = _snapshot(nat, G)
    rekey_info, table = _lib.PdlRekeyInfo(), nat.rank_table()
    assert nat._lib.pdl_get_rekey_info(nat._ctx, C.byref(rekey_info)) == _lib.PDL_OK
    p0 = nat.query_scores(*plain).as_dict()
    assert nat.last_query_rekey_info == dict(queries_rekeyed=0, letters_base=4, letters_max=4, key_bits_base=32, key_bits_max=32, records_rebased=0,
                                             rebase_ms=0.0)
    a = _check_against_oracle(nat, base, query, k, "first")
    ra = nat.last_query_rekey_info
    assert (ra["queries_rekeyed"], ra["letters_base"], ra["letters_max"], ra["key_bits_base"], ra["key_bits_max"]) == (1, 4, 5, 32, 38)
    assert ra["records_rebased"] == nat.last_query_info["records"] and ra["rebase_ms"] > 0
    H.assert_scores_equal(nat.query_scores(*plain).as_dict(), p0, "a plain query in between")
    _check_against_oracle(nat, base, other, k, "another alphabet")
    assert nat.last_query_rekey_info["letters_max"] == 6 and nat.last_query_rekey_info["key_bits_max"] == 42
    H.assert_scores_equal(nat.query_scores(*query).as_dict(), a, "the first again")
    nat.set_option("stage_timers", 0)
    H.assert_scores_equal(nat.query_scores(*query).as_dict(), a, "without stage timers")
    assert nat.last_query_rekey_info["rebase_ms"] == 0.0
    nat.set_option("stage_timers", 1)
    info = _lib.PdlRekeyInfo()
    assert nat._lib.pdl_get_rekey_info(nat._ctx, C.byref(info)) == _lib.PDL_OK and info.as_dict()["rekeyed"] == 0
    assert info.as_dict() == rekey_info.as_dict()                    # pdl_get_rekey_info does not move
    t2 = nat.rank_table()
    assert np.array_equal(t2[0], table[0]) and t2[1] == table[1]
    nat.score_all()                                                  # ("stage_timers" made the scores stale; the pass gives the same)
    after = _snapshot(nat, G)
    for g in range(G):
        H.assert_scores_equal(after["scores"][g], before["scores"][g], f"base genome {g}")
    assert all(np.array_equal(x, y) for x, y in zip(after["dictionary"], before["dictionary"]))
    assert after["costs"] == before["costs"] and after["cost"] == before["cost"]
    nat.close()


# ---- random seeds -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", list(range(S.SEED0, S.SEED0 + N_SEEDS)))
def test_random_seeds(seed):
    case = S.query_rekey_case(seed)
    assert S.classify(case) == "supported"
    k, base, query = case["k"], case["base"], case["query"]
    nat = _native(k, *base, options=REKEY)
    got = _check_against_oracle(nat, base, query, k, f"seed {seed}")
    rk = nat.last_query_rekey_info
    assert rk["queries_rekeyed"] == 1 and rk["letters_max"] == len(case["alphabet"]) + len(case["letters"]) + len(case["short_letter"])
    if seed % 3 == 0:                                                # ... and as a batch of the genome split in two, whole genome first
        genes = case["query_genes"]
        h = max(1, len(genes) // 2)
        halves = [_genes(*genes[:h]), _genes(*genes[h:])] if len(genes) > 1 else [_genes(*genes)]
        blocks = nat.query_batch([query] + halves)
        H.assert_scores_equal(blocks[0].as_dict(), got, f"seed {seed}: whole genome in a batch")
        for j, half in enumerate(halves):
            H.assert_scores_equal(blocks[1 + j].as_dict(), nat.query_scores(*half).as_dict(), f"seed {seed}: half {j}")
    nat.close()
