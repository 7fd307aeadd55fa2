"""pdl_remove_genomes on the GPU: a context shrunk by a compaction must be, bit for bit, the context pdl_preprocess leaves on
the remaining set.  Every pinned set pins a removal: splice an intruder genome into it, build the larger set, remove the
intruder — the reference's fixtures and digests must come out.  Beside that: a build of the remaining set on the device and the
CPU oracle, the identities with append and query, the fold of the last record, the refusals (which leave the context alone), a
fuzz range, the remove command end to end."""
import gzip
import json
import os

import numpy as np
import pytest

from tests import helpers as H
from tests.test_gpu_append import (_assert_oracle, _assert_same_context, _assert_snapshot, _check_digests, _genome, _pack, _prefix,
                                   _snapshot, _write_faa)
from tests.test_gpu_query import _native, _union
from tests.test_query_golden import load_case, union_arrays
from tests.test_remove_cpu import (POSITIONS, REMOVE_SEED0, REMOVE_SEEDS_DEFAULT, classify_removal, fuzz_case, intruder_genes,
                                   splice)

pytestmark = pytest.mark.gpu
N_SEEDS = int(os.environ.get("PDL_REMOVE_SEEDS", str(REMOVE_SEEDS_DEFAULT)))
BASE = json.loads((H.GOLDEN / "digests_baseline.json").read_text())


def _code(fn):
    from pandelos_amd import _lib
    with pytest.raises(_lib.PdlError) as e:
        fn()
    return e.value.code, str(e.value)


def _remaining(res, off, gen, removed):
    from pandelos_amd.remove import remaining_input
    return remaining_input(res, off, gen, removed)


def _remove_vs_rebuild(res, off, gen, k, removed, label, flags=0, options=(), oracle=True, edges=True, late=(), ora=None):
    """Build the whole set, remove `removed`, compare with a build of the remaining set (and the oracle on it).  `late`: options
    set between the build and the removal; the remaining set is built under what is in force at the end."""
    nat = _native(k, res, off, gen, flags=flags, options=options, late=late)
    whole = nat.cost.as_dict()
    nat.remove(removed)
    rest = _remaining(res, off, gen, removed)
    reb = _native(k, *rest, flags=flags, options=tuple(options) + tuple(late))
    _assert_same_context(nat, reb, label, edges=edges)
    if oracle and not flags:
        _assert_oracle(nat, *rest, k, label, ora=ora)
    info = nat.last_remove_info
    assert info["sequences"] == whole["sequences"] - reb.cost.sequences and info["residues"] == len(res) - len(rest[0]), label
    assert info["kmer_occurrences"] == whole["kmer_occurrences"] - reb.cost.kmer_occurrences, label
    assert info["records"] == whole["dictionary_records"] - reb.cost.dictionary_records, label
    reb.close()
    return nat


# ---- 1. the reference's fixtures, through an intruder ---------------------------------------------------------------------------
@pytest.mark.parametrize("position", POSITIONS)
@pytest.mark.parametrize("name", H.SMALL_CASES)
def test_fixture_with_an_intruder_removed_gives_the_fixture(name, position):
    from pandelos_amd import _lib
    res, off, gen, k, fx = H.load_small(name)
    G = int(gen.max()) + 1
    r2, o2, g2, gx = splice(res, off, gen, intruder_genes(res, off, 11), position)
    verdict = classify_removal(r2, o2, g2, k, [gx])
    assert verdict == ("undecodable" if name.endswith("_hash") else "ok"), verdict
    nat = _native(k, r2, o2, g2)
    assert nat.cost.genomes == G + 1
    if verdict == "ok":
        nat.remove([gx])
        assert nat.cost.genomes == G and nat.cost.sequences == len(gen) and nat.cost.residues == len(res)
        H.assert_scores_equal_fixture(lambda g: nat.generate_scores_part(g).as_dict(), fx, G, f"{name} {position}")
    else:
        snap = _snapshot(nat)
        c, msg = _code(lambda: nat.remove([gx]))
        assert c == _lib.PDL_ERR_UNSUPPORTED and "cannot be decoded" in msg and "hashed" in msg
        _assert_snapshot(nat, snap, f"{name} {position}: refused")
    nat.close()


# ---- 2. the reference's digests ---------------------------------------------------------------------------------------------------
def _with_genomes_in_the_middle(gs, extra, at):
    """`extra`'s genomes as genomes at .. at+r-1 of `gs` (both laid out genome after genome) -> arrays, the intruders' ids"""
    n = int((gs.genome_of < at).sum())
    cut, r = int(gs.offsets[n]), int(extra.genome_of.max()) + 1
    res = np.concatenate([gs.residues[:cut], extra.residues, gs.residues[cut:]])
    lens = np.concatenate([np.diff(gs.offsets.astype(np.int64))[:n], np.diff(extra.offsets.astype(np.int64)), np.diff(gs.offsets.astype(np.int64))[n:]])
    off = np.zeros(len(lens) + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    gen = np.concatenate([gs.genome_of[:n], extra.genome_of + at, gs.genome_of[n:] + r]).astype(np.uint32)
    return res, off, gen, list(range(at, at + r))


@pytest.mark.parametrize("name", ["salmonella7_standin", "mycoplasma64_standin"])
def test_intruder_in_the_middle_removed_matches_the_reference_digests(name):
    from pandelos_amd.pangene_native import PangeneNative
    d = BASE[name]
    gs = H.make_gene_set(**d["shape"])
    extra = H.make_gene_set(**{**d["shape"], "genomes": 1, "seed": d["shape"]["seed"] + 77})
    res, off, gen, ids = _with_genomes_in_the_middle(gs, extra, d["genomes"] // 2)
    nat = PangeneNative.from_arrays(d["k"], res, off, gen)
    nat.remove(ids)
    assert nat.cost.sequences == d["sequences"] and nat.cost.genomes == d["genomes"] and nat.cost.residues == len(gs.residues)
    _check_digests(nat, d, f"{name}: + 1 - 1")
    nat.close()


def test_four_intruders_removed_one_by_one_and_at_once_match_the_reference_digests():
    from pandelos_amd.pangene_native import PangeneNative
    name = "mycoplasma64_standin"
    d = BASE[name]
    gs = H.make_gene_set(**d["shape"])
    extra = H.make_gene_set(**{**d["shape"], "genomes": 4, "seed": 6499})
    res, off, gen, ids = _with_genomes_in_the_middle(gs, extra, 20)
    one = PangeneNative.from_arrays(d["k"], res, off, gen)
    for left in range(4, 0, -1):
        one.remove([ids[0] + (left - 1) // 2])             # (the ids close up after every removal)
        assert one.cost.genomes == 64 + left - 1
    _check_digests(one, d, "68 - 1 - 1 - 1 - 1")
    four = PangeneNative.from_arrays(d["k"], res, off, gen)
    four.remove(ids[::-1])
    _check_digests(four, d, "68 - 4")
    _assert_same_context(one, four, "one by one vs at once")
    one.close(); four.close()


# ---- 3. the same context as a build of the remaining set ------------------------------------------------------------------------
@pytest.mark.parametrize("seed,tier,tier0,protein,which", [(61, 10, 0, False, "first"), (62, 11, 1, True, "middle"), (63, 21, 0, True, "last"),
                                                           (64, 9, 1, False, "several")])
def test_mid_size_sets_equal_a_build_of_the_remaining_set(seed, tier, tier0, protein, which):
    from pandelos_amd.calculate_k import calculate_k
    from pandelos_amd.synth import make_gene_set
    rng = np.random.default_rng(seed)
    gs = make_gene_set(genomes=int(rng.integers(6, 24)), genes_per_genome=int(rng.integers(150, 400)), mean_len=int(rng.integers(80, 200)),
                       sub_rate=0.1, seed=seed, protein_like=protein)
    k = calculate_k(gs.residues)
    G = int(gs.genome_of.max()) + 1
    removed = {"first": [0], "middle": [G // 2], "last": [G - 1], "several": [G - 1, 0, G // 2, 1]}[which]
    _remove_vs_rebuild(gs.residues, gs.offsets, gs.genome_of, k, removed, f"seed {seed} tier {tier} {which}",
                       options=[("join_tier1", tier), ("join_tier0", tier0)]).close()


def test_65_protein_like_genomes_minus_one_equal_a_build_of_64():
    from pandelos_amd.synth import make_gene_set
    gs = make_gene_set(genomes=65, genes_per_genome=750, mean_len=370, sub_rate=0.25, seed=6465, protein_like=True)
    _remove_vs_rebuild(gs.residues, gs.offsets, gs.genome_of, 5, [31], "65-1", oracle=False).close()


# ---- 4. identities ------------------------------------------------------------------------------------------------------------------
def _small():
    from pandelos_amd.synth import make_gene_set
    gs = make_gene_set(genomes=7, genes_per_genome=90, mean_len=110, sub_rate=0.12, seed=8123, protein_like=True)
    return gs.residues, gs.offsets, gs.genome_of, 4


def test_append_then_remove_the_newcomer_is_the_base_build():
    res, off, gen, k = _small()
    base, A = _prefix(res, off, gen, 6), _genome(res, off, gen, 6, 7)[:2]
    nat, ref = _native(k, *base), _native(k, *base)
    nat.score_all()
    nat.append(*A)
    nat.remove([6])
    _assert_same_context(nat, ref, "base + A - A")
    assert nat.last_remove_info["residues"] == len(A[0]) and nat.last_remove_info["kmer_occurrences"] == nat.last_append_info["kmer_occurrences"]
    assert nat.last_remove_info["records"] == nat.last_append_info["records"]
    nat.close(); ref.close()


def test_remove_the_last_genome_then_append_it_again_matches_the_reference_digests():
    from pandelos_amd.pangene_native import PangeneNative
    d = BASE["mycoplasma64_standin"]
    gs = H.make_gene_set(**d["shape"])
    res, off, gen = gs.residues, gs.offsets, gs.genome_of
    nat = PangeneNative.from_arrays(d["k"], res, off, gen)
    nat.remove([63])
    assert nat.cost.genomes == 63
    nat.append(*_genome(res, off, gen, 63, 64)[:2])
    _check_digests(nat, d, "64 - 1 + 1")
    nat.close()


def test_query_remove_query_append_remove():
    from oracle import binding as ob
    res, off, gen, k = _small()
    upto6 = _prefix(res, off, gen, 6)
    B = _genome(res, off, gen, 6, 7)[:2]
    nat = _native(k, *upto6)
    H.assert_scores_equal(nat.query_scores(*B).as_dict(), ob.Oracle(res, off, gen, k).scores(6), "query B")
    nat.remove([2])
    rest = _remaining(*upto6, [2])
    _assert_oracle(nat, *rest, k, "6 - genome 2")
    r2, o2, g2, G = _union(rest, B)
    ora = ob.Oracle(r2, o2, g2, k)
    H.assert_scores_equal(nat.query_scores(*B).as_dict(), ora.scores(G), "query B after the removal")
    assert nat.last_query_info["genome_cost"] == ora.genome_cost(G)
    nat.append(*B)
    _assert_oracle(nat, r2, o2, g2, k, "6 - genome 2 + B")
    nat.remove([0, G])
    _assert_oracle(nat, *_remaining(r2, o2, g2, [0, G]), k, "... - genome 0 - B")
    nat.close()


def test_base_built_from_device_input_that_is_gone_by_the_time_of_the_removal():
    import torch
    from pandelos_amd.pangene_native import PangeneNative
    res, off, gen, k = _small()
    base, A = _prefix(res, off, gen, 6), _genome(res, off, gen, 6, 7)[:2]
    rb, ob_, gb = base
    dev = torch.device("cuda", 0)
    t_res = torch.from_numpy(np.concatenate([rb, np.zeros(32, np.uint8)])).to(dev)
    t_off = torch.from_numpy(ob_.astype(np.int64)).to(dev)
    t_gen = torch.from_numpy(gb.astype(np.int32)).to(dev)
    nat = PangeneNative.from_device(k, t_res.data_ptr(), t_off.data_ptr(), t_gen.data_ptr(), len(gb), len(rb))
    nat.append(*A)
    torch.cuda.synchronize()
    t_res.fill_(0); t_off.fill_(0); t_gen.fill_(0x7fffffff)       # whoever still read the caller's buffers would notice
    torch.cuda.synchronize()
    del t_res, t_off, t_gen
    torch.cuda.empty_cache()
    nat.remove([1, 4])
    reb = _native(k, *_remaining(res, off, gen, [1, 4]))
    _assert_same_context(nat, reb, "device input, append, remove")
    nat.close(); reb.close()
    # ... and straight after the device build, the caller's buffers still there (as the header asks)
    t_res = torch.from_numpy(np.concatenate([rb, np.zeros(32, np.uint8)])).to(dev)
    t_off = torch.from_numpy(ob_.astype(np.int64)).to(dev)
    t_gen = torch.from_numpy(gb.astype(np.int32)).to(dev)
    nat = PangeneNative.from_device(k, t_res.data_ptr(), t_off.data_ptr(), t_gen.data_ptr(), len(gb), len(rb), keepalive=(t_res, t_off, t_gen))
    nat.remove([0])
    reb = _native(k, *_remaining(*base, [0]))
    _assert_same_context(nat, reb, "device input, remove")
    nat.close(); reb.close()


def test_families_after_a_removal_are_those_of_the_remaining_set():
    res, off, gen, k = _small()
    nat = _native(k, res, off, gen)
    before = nat.generate_families()
    nat.remove([3])
    reb = _native(k, *_remaining(res, off, gen, [3]))
    a, b = nat.generate_families(), reb.generate_families()
    assert a["sequences"] == reb.cost.sequences < before["sequences"]
    for key in b:
        assert np.array_equal(a[key], b[key]), key
    nat.close(); reb.close()


def test_canonical_order_flag():
    from pandelos_amd import _lib
    res, off, gen, k = _small()
    _remove_vs_rebuild(res, off, gen, k, [5, 2], "canonical order", flags=_lib.PDL_FLAG_CANONICAL_ORDER).close()


# ---- 5. the fold of the last record moves ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["q1a_query_max_folds_into_base_group", "q1b_base_fold_undone", "q1c_base_last_folds_into_query_group",
                                  "q1d_query_joins_base_max_group"])
def test_query_fixture_union_minus_the_query_is_the_base_build(name):
    from pandelos_amd.pangene_native import PangeneNative
    fx, base, query, k, G = load_case(name)
    res, off, gen, _ = union_arrays(base, query)
    nat = _native(k, res, off, gen)
    nat.remove([G])
    ref = PangeneNative(k, base)
    _assert_same_context(nat, ref, name)
    _assert_oracle(nat, *base.flatten(), k, name)
    nat.close(); ref.close()


def test_the_largest_kmer_lives_only_in_the_removed_genome():
    rng = np.random.default_rng(5)
    mid = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    seqs = [mid[rng.integers(0, 19, int(rng.integers(40, 90)))].tobytes() for _ in range(40)]      # no Y among them ...
    seqs[13] = seqs[13] + b"YYYA"                                                                   # ... one gene of the remaining set holds it
    seqs += [b"YYYYYY" + seqs[0], b"AAYYYY"]                                                        # the largest k-mers: the removed genome's
    gen = [i // 10 for i in range(40)] + [4, 4]
    res, off, g = _pack(seqs, gen)
    for removed in ([4], [4, 0]):
        _remove_vs_rebuild(res, off, g, 4, removed, f"largest k-mer leaves with {removed}").close()


# ---- 6. refusals leave the context alone ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was():
    import ctypes as C
    import torch
    from pandelos_amd import _lib
    from pandelos_amd.pangene_native import PangeneNative
    res, off, gen, k = _small()
    G = int(gen.max()) + 1

    fresh = PangeneNative.open()
    assert _code(lambda: fresh.remove([0]))[0] == _lib.PDL_ERR_STATE
    fresh.close()
    cplx = PangeneNative.from_arrays(k, res, off, gen, only_complexity=True)
    assert _code(lambda: cplx.remove([0]))[0] == _lib.PDL_ERR_STATE
    assert cplx.cost.genomes == G
    cplx.close()
    low = PangeneNative.open()
    low.set_option("low_memory", 1)
    low.preprocess(k, res, off, gen)
    assert _code(lambda: low.remove([0]))[0] == _lib.PDL_ERR_STATE
    low.close()
    shard = _native(k, res, off, gen, shard=[0, 2])
    before = shard.generate_scores_part(2).as_dict()
    assert _code(lambda: shard.remove([1]))[0] == _lib.PDL_ERR_STATE
    H.assert_scores_equal(shard.generate_scores_part(2).as_dict(), before, "shard")
    shard.close()
    dev = torch.device("cuda", 0)
    t_res = torch.from_numpy(np.concatenate([res, np.zeros(32, np.uint8)])).to(dev)
    t_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    t_gen = torch.from_numpy(gen.astype(np.int32)).to(dev)
    dist = PangeneNative.open()
    dist.dist_preprocess_begin(k, t_res.data_ptr(), t_off.data_ptr(), t_gen.data_ptr(), len(gen), len(res), 1, 0)
    assert _code(lambda: dist.remove([0]))[0] == _lib.PDL_ERR_STATE
    dist.close()

    nat = _native(k, res, off, gen)
    snap = _snapshot(nat)
    assert _code(lambda: nat.remove([]))[0] == _lib.PDL_ERR_ARGUMENT                                    # NULL list / count == 0
    assert _code(lambda: nat.remove([G]))[0] == _lib.PDL_ERR_ARGUMENT                                   # id >= G
    assert _code(lambda: nat.remove([1, 3, 1]))[0] == _lib.PDL_ERR_ARGUMENT                             # named twice
    assert _code(lambda: nat.remove(list(range(G))))[0] == _lib.PDL_ERR_ARGUMENT                        # every genome
    one = np.array([0], np.uint32)
    assert nat._lib.pdl_remove_genomes(nat._ctx, one.ctypes.data, 0, None, None) == _lib.PDL_ERR_ARGUMENT
    assert nat._lib.pdl_remove_genomes(nat._ctx, None, 1, None, None) == _lib.PDL_ERR_ARGUMENT
    assert nat._lib.pdl_remove_genomes(None, one.ctypes.data, 1, None, None) == _lib.PDL_ERR_ARGUMENT
    _assert_snapshot(nat, snap, "after the argument refusals")
    # ... and it still takes a removal, and a preprocess afterwards behaves as on a fresh context
    nat.remove([G - 1])
    _assert_oracle(nat, *_prefix(res, off, gen, G - 1), k, "removal after the refusals")
    nat.preprocess(k, res, off, gen)
    _assert_snapshot(nat, snap[:-1] + (None,), "preprocess after a removal")
    nat.close()


def test_alphabet_and_empty_refusals_leave_the_context_as_it_was():
    from pandelos_amd import _lib
    rng = np.random.default_rng(17)
    mid = np.frombuffer(b"ACDEFGHIKLMNPQRSTVW", np.uint8)
    body = [mid[rng.integers(0, len(mid), int(rng.integers(30, 80)))].tobytes() for _ in range(24)]
    k = 4
    # genome 0: the only Y of a k-mer; genome 1 keeps a Y in a gene shorter than k; genome 2: plain; genome 3: short genes only
    seqs = [body[0] + b"YA", b"AY"] + body[1:9] + body[9:] + [b"ACD", b"", b"EF"]
    gen = [0, 1] + [1] * 8 + [2] * 15 + [3] * 3
    res, off, g = _pack(seqs, gen)
    nat = _native(k, res, off, g)
    snap = _snapshot(nat)
    c, msg = _code(lambda: nat.remove([0]))
    assert c == _lib.PDL_ERR_UNSUPPORTED and "0x59" in msg and "'Y'" in msg and "conservative" in msg and "shorter than k=4" in msg, msg
    assert classify_removal(res, off, g, k, [0]) == "alphabet"
    c, msg = _code(lambda: nat.remove([0, 1]))                      # now the letter is gone altogether: the same refusal
    assert c == _lib.PDL_ERR_UNSUPPORTED and "'Y'" in msg
    c, msg = _code(lambda: nat.remove([0, 1, 2]))                   # what remains has no k-mer
    assert c == _lib.PDL_ERR_EMPTY and "dictionary is empty" in msg
    assert classify_removal(res, off, g, k, [0, 1, 2]) == "empty"
    _assert_snapshot(nat, snap, "after the alphabet and empty refusals")
    nat.remove([3, 2])                                              # ... and this one goes through
    _assert_oracle(nat, *_remaining(res, off, g, [3, 2]), k, "removal after the refusals")
    nat.close()


def test_remove_info_and_timings_describe_the_removal():
    res, off, gen, k = _small()
    nat = _native(k, res, off, gen)
    nat.score_all()
    nat.remove([2])
    info, tm = nat.last_remove_info, nat.timings()
    assert info["compact_ms"] > 0 and info["device_ms"] > info["compact_ms"]
    assert tm["preprocess_total_ms"] == info["device_ms"] and tm["sort_rank_ms"] == info["compact_ms"]
    assert tm["hist_ms"] == 0 and tm["rank_ms"] == 0 and tm["dict_ms"] > 0 and tm["join_ms"] == 0 and tm["emitted_cells"] == 0
    nat.close()


# ---- 7. random small sets -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", list(range(REMOVE_SEED0, REMOVE_SEED0 + N_SEEDS)))
def test_random_small_sets_equal_the_oracle_or_are_refused(seed):
    from oracle import binding as ob
    from pandelos_amd import _lib
    from pandelos_amd.pangene_native import PangeneNative
    res, off, gen, k, removed, verdict = fuzz_case(seed)
    if verdict == "skip":
        pytest.skip("one genome only: nothing to remove")
    nat = PangeneNative.open()
    if int(np.maximum(np.diff(off.astype(np.int64)) - k + 1, 0).sum()) == 0:        # the set itself has no k-mer
        assert verdict == "empty" and _code(lambda: nat.preprocess(k, res, off, gen))[0] == _lib.PDL_ERR_EMPTY
        assert _code(lambda: nat.remove(removed))[0] == _lib.PDL_ERR_STATE
        nat.close()
        return
    nat.preprocess(k, res, off, gen)
    if verdict == "ok":
        nat.remove(removed)
        rest = _remaining(res, off, gen, removed)
        ora = ob.Oracle(*rest, k)
        assert nat.cost.genomes == ora.genomes and nat.cost.total_cost == ora.total_cost and nat.cost.residues == len(rest[0])
        for g in range(ora.genomes):
            H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), ora.scores(g), f"seed {seed} genome {g}")
            assert nat.genome_cost(g) == ora.genome_cost(g)
    else:
        before = (nat.cost.as_dict(), nat.dictionary(), [nat.generate_scores_part(g).as_dict() for g in range(nat.cost.genomes)])
        c, _ = _code(lambda: nat.remove(removed))
        assert c == (_lib.PDL_ERR_EMPTY if verdict == "empty" else _lib.PDL_ERR_UNSUPPORTED), (verdict, c)
        assert nat.cost.as_dict() == before[0] and all(np.array_equal(x, y) for x, y in zip(nat.dictionary(), before[1]))
        for g, want in enumerate(before[2]):
            H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), want, f"seed {seed} genome {g} after the refusal")
    nat.close()


# ---- 8. end to end ----------------------------------------------------------------------------------------------------------------------
def test_remove_command_replaces_the_last_genome_and_writes_the_canonical_net(tmp_path):
    from pandelos_amd import remove as R
    name = "mycoplasma64_standin"
    gs = H.make_gene_set(**BASE[name]["shape"])
    full, last, net = tmp_path / "full.faa", tmp_path / "last.faa", tmp_path / "out.net"
    _write_faa(gs, full, 0, 64); _write_faa(gs, last, 63, 64)
    assert R.main(["-i", str(full), "-k", str(BASE[name]["k"]), "-r", "G63", "-a", str(last), "-o", str(net)]) == 0
    want = gzip.open(H.GOLDEN / "net" / f"{name}.net.gz", "rb").read()
    assert net.read_bytes() == want


def test_remove_command_rebuilds_when_the_removal_is_refused(tmp_path, capsys):
    from pandelos_amd import pangenes as P
    from pandelos_amd import remove as R
    rng = np.random.default_rng(23)
    mid = np.frombuffer(b"ACDEFGHIKLMNPQRSTVW", np.uint8)
    fams = [mid[rng.integers(0, len(mid), 60)] for _ in range(8)]          # every genome holds a copy of each, a few letters changed

    def copy_of(f):
        g = f.copy()
        m = rng.random(len(g)) < 0.05
        g[m] = mid[rng.integers(0, len(mid), int(m.sum()))]
        return g.tobytes()
    recs = [(b"G%d" % (i // 8), b"g%d" % i, copy_of(fams[i % 8]) + (b"YYYY" if i // 8 == 1 else b"")) for i in range(32)]
    full, rest, net, want = tmp_path / "full.faa", tmp_path / "rest.faa", tmp_path / "out.net", tmp_path / "want.net"
    full.write_bytes(b"".join(b"%s\t%s\tp\n%s\n" % r for r in recs))
    rest.write_bytes(b"".join(b"%s\t%s\tp\n%s\n" % r for r in recs if r[0] != b"G1"))
    assert R.main(["-i", str(full), "-k", "4", "-r", "G1", "-o", str(net)]) == 0
    out = capsys.readouterr().out
    assert "'Y'" in out and "rebuilding from the remaining records" in out
    assert P.main(["-i", str(rest), "-k", "4", "-o", str(want)]) == 0
    assert net.read_bytes() == want.read_bytes() and len(want.read_bytes()) > 0
