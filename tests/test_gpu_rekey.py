"""Option alphabet_rekey on the GPU: an append that brings letters the base lacks and a removal after which letters are gone leave,
bit for bit, the context pdl_preprocess leaves on the union / the remaining set — against a fresh build on the device and the CPU
oracle; the key width follows the alphabet up and down; what cannot be re-keyed is refused with the context untouched; the letters
of genes shorter than k; round trips; a random range in which no seed may be skipped or refused; the two commands."""
import os

import numpy as np
import pytest

from tests import helpers as H
from tests.test_gpu_append import _assert_oracle, _assert_same_context, _assert_snapshot, _snapshot
from tests.test_gpu_query import _native, _union
from tests.test_query_golden import load_case
from tests.test_rekey_cpu import (REKEY_SEED0, REKEY_SEEDS_DEFAULT, classify_rekey, family_genes, kmers, pack, rekey_case,
                                  with_letters)

pytestmark = pytest.mark.gpu
N_SEEDS = int(os.environ.get("PDL_REKEY_SEEDS", str(REKEY_SEEDS_DEFAULT)))
A19 = b"ACDEFGHIKLMNPQRSTVW"
ON = [("alphabet_rekey", 1)]
TILE = 1024                                             # keys of one workgroup's pass over the stream (256 threads, four keys each)


def _code(fn):
    from pandelos_amd import _lib
    with pytest.raises(_lib.PdlError) as e:
        fn()
    return e.value.code, str(e.value)


def _remaining(res, off, gen, removed):
    from pandelos_amd.remove import remaining_input
    return remaining_input(res, off, gen, removed)


def _family(alphabet, k, genomes=4, genes=10, lo=30, hi=80, seed=5, sub=0.1):
    """-> (base arrays of `genomes` related genomes, the genes of one more).  The base's stream is longer than a re-key tile and
    no multiple of 4 keys: tile edges and the unaligned tail are met."""
    fam = family_genes(alphabet, genomes + 1, genes, lo, hi, seed, sub)
    seqs = [g for gs in fam[:genomes] for g in gs]
    gen = [i for i in range(genomes) for _ in range(genes)]
    while kmers(pack(seqs, gen)[1], k) % 4 == 0:
        seqs[-1] += alphabet[:1]
    base = pack(seqs, gen)
    assert kmers(base[1], k) > TILE and kmers(base[1], k) % 4
    return base, fam[genomes]


def _genes(seqs):
    return pack(seqs, [0] * len(seqs))[:2]


def _assert_dictionary_is_the_oracles(nat, res, off, gen, k, label, ora=None):
    from oracle import binding as ob
    d = (ora or ob.Oracle(res, off, gen, k)).dictionary()
    ranks, seqs, counts = nat.dictionary()
    assert np.array_equal(ranks, d["rank"]) and np.array_equal(seqs, d["seq"]) and np.array_equal(counts, d["count"]), f"{label}: dictionary vs oracle"


def _check_info(nat, rekeyed, before, after, m, label, timed=True):
    """last_rekey_info against the letters and rank_bits of the two sets and the length of the re-keyed stream.  `timed`: the
    stages' events are on (option "stage_timers", the default); without them the re-key reports no time."""
    ri = nat.last_rekey_info
    assert ri["rekeyed"] == int(rekeyed), (label, ri)
    assert ri["letters_before"] == before[0] and ri["key_bits_before"] == before[1], (label, ri)
    assert ri["letters_after"] == after[0] and ri["key_bits_after"] == after[1], (label, ri)
    assert ri["keys_rewritten"] == (m if rekeyed else 0), (label, ri)
    assert (ri["rekey_ms"] > 0) == bool(rekeyed and timed), (label, ri)


def _fresh_options(options, late):
    """what the context to compare with is built under: everything in force at the end but "alphabet_rekey", which a build of
    the final set has no use for"""
    return tuple(o for o in tuple(options) + tuple(late) if o[0] != "alphabet_rekey")


def _append_vs_union(base, query, k, label, rekeyed=True, options=ON, late=(), ora=None):
    """`late`: options set between the base's build and the append (tests/option_forms.py); `ora`: the oracle on the union where
    the caller has it.  With "stage_timers" 0 in force the stages report no times: only the total is compared."""
    timed = dict(_fresh_options(options, late)).get("stage_timers", 1) != 0
    res, off, gen, G = _union(base, query)
    nat = _native(k, *base, options=options, late=late)
    before = (len(np.unique(base[0])), nat.cost.rank_bits)
    m0 = nat.cost.kmer_occurrences
    nat.append(*query)
    uni = _native(k, res, off, gen, options=_fresh_options(options, late))
    _assert_same_context(nat, uni, label)
    _assert_oracle(nat, res, off, gen, k, label, ora=ora)
    _assert_dictionary_is_the_oracles(nat, res, off, gen, k, label, ora=ora)
    _check_info(nat, rekeyed, before, (len(np.unique(res)), uni.cost.rank_bits), m0, label, timed)
    tm, info, ri = nat.timings(), nat.last_append_info, nat.last_rekey_info
    assert tm["preprocess_total_ms"] == info["device_ms"], label
    # the re-key's time is part of the sort's share: rank + (sort + merge + re-key) = what the infos report; K-hist is the build's alone
    assert not timed or abs(tm["sort_rank_ms"] + tm["rank_ms"] - info["rank_sort_ms"] - info["merge_ms"] - ri["rekey_ms"]) < 1e-3, (label, tm, info, ri)
    assert tm["hist_ms"] == 0, (label, tm)
    uni.close()
    return nat


def _remove_vs_rebuild(res, off, gen, k, removed, label, rekeyed=True, options=ON, late=(), ora=None):
    timed = dict(_fresh_options(options, late)).get("stage_timers", 1) != 0
    nat = _native(k, res, off, gen, options=options, late=late)
    before = (len(np.unique(res)), nat.cost.rank_bits)
    nat.remove(removed)
    rest = _remaining(res, off, gen, removed)
    reb = _native(k, *rest, options=_fresh_options(options, late))
    _assert_same_context(nat, reb, label)
    _assert_oracle(nat, *rest, k, label, ora=ora)
    _assert_dictionary_is_the_oracles(nat, *rest, k, label, ora=ora)
    _check_info(nat, rekeyed, before, (len(np.unique(rest[0])), reb.cost.rank_bits), reb.cost.kmer_occurrences, label, timed)
    tm, info, ri = nat.timings(), nat.last_remove_info, nat.last_rekey_info
    assert tm["preprocess_total_ms"] == info["device_ms"], label
    # the compaction and the re-key are the removal's "sort"; nothing is ranked or counted
    assert not timed or abs(tm["sort_rank_ms"] - info["compact_ms"] - ri["rekey_ms"]) < 1e-3, (label, tm, info, ri)
    assert tm["hist_ms"] == 0 and tm["rank_ms"] == 0, (label, tm)
    reb.close()
    return nat


# ---- 1. append, the key width stays --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letters", [b"Y", b"B", b"*", b"BZ"], ids=["above", "between", "below", "two"])
def test_append_with_new_letters(letters):
    base, new = _family(A19, 4)
    query = _genes([with_letters(g, letters, 40 + j) for j, g in enumerate(new)])
    assert set(letters) <= set(query[0].tolist())
    _append_vs_union(base, query, 4, f"+ {letters!r}").close()


def test_append_whose_only_new_letter_sits_in_a_gene_shorter_than_k():
    """No new k-mer holds the letter, but B grows as in a build and every key of the base changes."""
    base, new = _family(A19, 4)
    _append_vs_union(base, _genes(new + [b"AY"]), 4, "Y in a short gene").close()


def test_append_without_any_kmer_but_with_a_new_letter():
    base, _ = _family(A19, 4)
    nat = _append_vs_union(base, _genes([b"AY", b"", b"YC"]), 4, "no k-mer, new letter")
    assert nat.last_append_info["kmer_occurrences"] == 0
    nat.close()


def test_append_without_a_new_letter_does_not_rekey():
    base, new = _family(A19, 4)
    _append_vs_union(base, _genes(new), 4, "same alphabet", rekeyed=False).close()


# ---- 2. append, the key width grows ---------------------------------------------------------------------------------------------------
def test_acgt_k16_plus_n_goes_from_32_to_38_bit_keys():
    base, new = _family(b"ACGT", 16)
    query = _genes([with_letters(g, b"N", 50 + j, every=25) for j, g in enumerate(new)])
    nat = _append_vs_union(base, query, 16, "ACGT + N")
    ri = nat.last_rekey_info
    assert (ri["key_bits_before"], ri["key_bits_after"], ri["letters_before"], ri["letters_after"]) == (32, 38, 4, 5)
    nat.close()


def test_two_letters_k32_plus_a_third():
    base, new = _family(b"AC", 32, lo=50, sub=0.02)
    query = _genes([with_letters(g, b"G", 60 + j, every=40) for j, g in enumerate(new)])
    nat = _append_vs_union(base, query, 32, "AC + G")
    assert nat.last_rekey_info["key_bits_before"] == 32 and nat.last_rekey_info["key_bits_after"] > 32
    nat.close()


def test_64_bit_keys_on_both_sides_and_a_key_in_three_parts():
    """k = 27: ACGT keys (2^54) are cut into 16 + 11 digits on the way up, ACGTN keys (5^27) into 13 + 13 + 1 on the way down."""
    base, new = _family(b"ACGT", 27, lo=50, sub=0.03)
    query = _genes([with_letters(g, b"N", 50 + j, every=40) for j, g in enumerate(new)])
    nat = _append_vs_union(base, query, 27, "ACGT + N, k = 27")
    assert nat.last_rekey_info["key_bits_before"] == 54 and nat.last_rekey_info["key_bits_after"] == 63
    nat.remove([4])
    ri = nat.last_rekey_info
    assert (ri["rekeyed"], ri["letters_before"], ri["letters_after"], ri["key_bits_after"]) == (1, 5, 4, 54)
    fresh = _native(27, *base)
    _assert_same_context(nat, fresh, "and back")
    _assert_dictionary_is_the_oracles(nat, *base, 27, "and back")
    nat.close(); fresh.close()


# ---- 3. append, refused: the context stays as it was ------------------------------------------------------------------------------------
@pytest.mark.parametrize("alphabet,add,k", [(A19, b"Y", 15), (b"ABCDEFGHIJKLMNOPQRSTUV", b"WX", 14)], ids=["20^15", "24^14"])
def test_a_union_whose_ranks_would_wrap_is_refused(alphabet, add, k):
    from pandelos_amd import _lib
    base, new = _family(alphabet, k, genes=8, lo=40)
    assert len(alphabet) ** k < 1 << 64 <= (len(alphabet) + len(add)) ** k
    nat = _native(k, *base, options=ON)
    snap = _snapshot(nat)
    c, msg = _code(lambda: nat.append(*_genes([with_letters(g, add, 70 + j) for j, g in enumerate(new)])))
    assert c == _lib.PDL_ERR_UNSUPPORTED and "union's ranks" in msg and f"{len(alphabet) + len(add)} letters" in msg, msg
    _assert_snapshot(nat, snap, "after the refusal")
    nat.append(*_genes(new))                                        # a legal append still goes through
    res, off, gen, _ = _union(base, _genes(new))
    _assert_oracle(nat, res, off, gen, k, "append after the refusal")
    nat.close()


def test_a_hashed_base_is_refused():
    from pandelos_amd import _lib
    fx, base, query, k, G = load_case("hash_fallback_20_letters_k16")
    b = base.flatten()
    rq, oq, _ = query.flatten()
    nat = _native(k, *b, options=ON)
    assert nat.cost.hash_fallback == 1
    snap = _snapshot(nat)
    bad = rq.copy()
    assert ord("*") not in set(b[0].tolist())
    bad[len(bad) // 2] = ord("*")
    c, msg = _code(lambda: nat.append(bad, oq))
    assert c == _lib.PDL_ERR_UNSUPPORTED and "base's ranks" in msg and "hashed" in msg and "0x2a" in msg, msg
    _assert_snapshot(nat, snap, "after the refusal")
    nat.append(rq, oq)
    res, off, gen, _ = _union(b, (rq, oq))
    _assert_oracle(nat, res, off, gen, k, "append after the refusal")
    nat.close()


# ---- 4. remove ------------------------------------------------------------------------------------------------------------------------
def _set_with_a_special_genome(alphabet, letters, k, special, **kw):
    """A family over `alphabet` of which genome `special` also holds `letters`."""
    every = kw.pop("every", 9)
    (res, off, gen), _ = _family(alphabet, k, **kw)
    seqs = [res[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(gen))]
    seqs = [with_letters(s, letters, 80 + i, every=every) if gen[i] == special else s for i, s in enumerate(seqs)]
    return pack(seqs, gen)


def test_the_only_genome_with_y_leaves():
    res, off, gen = _set_with_a_special_genome(A19, b"Y", 4, 1, genomes=5)
    _remove_vs_rebuild(res, off, gen, 4, [1], "- Y").close()


def _y_in_a_short_gene():
    """The set of test_gpu_remove's alphabet refusals: genome 0 holds the only Y of a k-mer, genome 1 keeps a Y in a gene shorter
    than k, genome 3 has short genes only."""
    rng = np.random.default_rng(17)
    mid = np.frombuffer(A19, np.uint8)
    body = [mid[rng.integers(0, len(mid), int(rng.integers(30, 80)))].tobytes() for _ in range(24)]
    seqs = [body[0] + b"YA", b"AY"] + body[1:9] + body[9:] + [b"ACD", b"", b"EF"]
    return pack(seqs, [0, 1] + [1] * 8 + [2] * 15 + [3] * 3)


def test_y_surviving_in_a_short_gene_of_a_genome_that_stays_needs_no_rekey():
    res, off, gen = _y_in_a_short_gene()
    _remove_vs_rebuild(res, off, gen, 4, [0], "Y stays in a short gene", rekeyed=False).close()
    _remove_vs_rebuild(res, off, gen, 4, [0, 1], "Y leaves altogether").close()


def test_acgtn_k16_without_its_n_genome_goes_from_64_to_32_bit_keys():
    res, off, gen = _set_with_a_special_genome(b"ACGT", b"N", 16, 2, genomes=5, every=25)
    nat = _remove_vs_rebuild(res, off, gen, 16, [2], "ACGTN - N")
    ri = nat.last_rekey_info
    assert (ri["key_bits_before"], ri["key_bits_after"], ri["letters_before"], ri["letters_after"]) == (38, 32, 5, 4)
    nat.close()


def test_what_remains_has_one_letter():
    rng = np.random.default_rng(3)
    poly = [b"A" * int(n) for n in rng.integers(30, 80, 30)]
    other = [g for gs in family_genes(b"ACDE", 2, 8, 30, 80, 9) for g in gs]
    res, off, gen = pack(poly + other, [0] * len(poly) + [1] * 8 + [2] * 8)
    assert kmers(off[:len(poly) + 1], 4) > TILE
    nat = _remove_vs_rebuild(res, off, gen, 4, [1, 2], "poly-A remains")
    assert nat.last_rekey_info["letters_after"] == 1 and nat.dictionary()[0].max() == 0
    nat.close()


def test_what_remains_has_no_kmer():
    from pandelos_amd import _lib
    base, _ = _family(A19, 4)
    res, off, gen = base
    seqs = [res[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(gen))] + [b"AY", b"ACD", b""]
    res, off, gen = pack(seqs, list(gen) + [4] * 3)
    nat = _native(4, res, off, gen, options=ON)
    snap = _snapshot(nat)
    c, msg = _code(lambda: nat.remove([0, 1, 2, 3]))
    assert c == _lib.PDL_ERR_EMPTY and "dictionary is empty" in msg
    _assert_snapshot(nat, snap, "after PDL_ERR_EMPTY")
    nat.close()


# ---- 5. the option set only after the build ------------------------------------------------------------------------------------------
def test_option_set_after_the_build():
    from pandelos_amd import _lib
    res, off, gen = _set_with_a_special_genome(A19, b"Y", 4, 1, genomes=5)
    nat = _native(4, res, off, gen)
    snap = _snapshot(nat)
    nat.set_option("alphabet_rekey", 1)                             # (no bearing on the scores: the snapshot holds)
    c, msg = _code(lambda: nat.remove([1]))
    assert c == _lib.PDL_ERR_UNSUPPORTED and "alphabet_rekey" in msg and "set it before pdl_preprocess" in msg, msg
    _assert_snapshot(nat, snap, "after the refusal")
    _, new = _family(A19, 4)
    query = _genes([with_letters(g, b"Z*", 90 + j) for j, g in enumerate(new)])
    nat.append(*query)                                              # an append needs no table of short genes
    u = _union((res, off, gen), query)[:3]
    uni = _native(4, *u)
    _assert_same_context(nat, uni, "append, option set late")
    assert nat.last_rekey_info["rekeyed"] == 1 and nat.last_rekey_info["letters_after"] == 22
    nat.close(); uni.close()


# ---- 6. round trips ---------------------------------------------------------------------------------------------------------------------
def test_append_a_new_letter_then_remove_it_again():
    base, new = _family(A19, 4)
    query = _genes([with_letters(g, b"Y", 40 + j) for j, g in enumerate(new)] + [b"BB"])
    nat = _native(4, *base, options=ON)
    nat.append(*query)
    assert nat.last_rekey_info["letters_after"] == 21
    nat.remove([4])
    assert nat.last_rekey_info["rekeyed"] == 1 and nat.last_rekey_info["letters_after"] == 19
    fresh = _native(4, *base)
    _assert_same_context(nat, fresh, "append + remove")
    _assert_oracle(nat, *base, 4, "append + remove")
    nat.close(); fresh.close()


def test_remove_the_genome_with_a_letter_then_append_it_back():
    res, off, gen = _set_with_a_special_genome(A19, b"Y", 4, 3)
    n = int((gen < 3).sum())
    last = (res[int(off[n]):].copy(), (off[n:] - off[n]).astype(np.uint64))
    nat = _native(4, res, off, gen, options=ON)
    nat.remove([3])
    assert nat.last_rekey_info["rekeyed"] == 1
    nat.append(*last)
    assert nat.last_rekey_info["rekeyed"] == 1
    whole = _native(4, res, off, gen)
    _assert_same_context(nat, whole, "remove + append")
    _assert_oracle(nat, res, off, gen, 4, "remove + append")
    nat.close(); whole.close()


def _same_dict(a, b, label):
    assert a.keys() == b.keys(), label
    for key in b:
        if isinstance(b[key], np.ndarray):
            assert a[key].dtype == b[key].dtype and H.raw(a[key]).tobytes() == H.raw(b[key]).tobytes(), f"{label}: {key}"
        else:
            assert a[key] == b[key], f"{label}: {key}"


def test_a_rekeyed_context_serves_queries_placements_families_and_appends():
    from oracle import binding as ob
    fam = family_genes(A19, 7, 10, 30, 80, 21)
    base = pack([g for gs in fam[:4] for g in gs], [i for i in range(4) for _ in range(10)])
    with_y = _genes([with_letters(g, b"Y", 40 + j) for j, g in enumerate(fam[4])])
    q1, q2 = _genes(fam[5]), _genes([with_letters(g, b"Y", 50 + j) for j, g in enumerate(fam[6])])
    nat = _native(4, *base, options=ON)
    nat.append(*with_y)
    u5 = _union(base, with_y)[:3]
    fresh = _native(4, *u5)
    u6 = _union(u5, q1)
    H.assert_scores_equal(nat.query_scores(*q1).as_dict(), ob.Oracle(*u6[:3], 4).scores(5), "query on the re-keyed context")
    _same_dict(nat.generate_families(), fresh.generate_families(), "families")
    _same_dict(nat.place_query(*q2), fresh.place_query(*q2), "placement")
    nat.append(*q1)                                                  # a plain append behind the re-keyed one
    assert nat.last_rekey_info["rekeyed"] == 0
    _assert_oracle(nat, *u6[:3], 4, "plain append behind")
    uni = _native(4, *u6[:3])
    _assert_same_context(nat, uni, "plain append behind")
    nat.close(); fresh.close(); uni.close()


# ---- 7. the option off ---------------------------------------------------------------------------------------------------------------------
def test_option_off_refuses_as_ever():
    from pandelos_amd import _lib
    base, new = _family(A19, 4)
    nat = _native(4, *base, options=[("alphabet_rekey", 0)])
    c, msg = _code(lambda: nat.append(*_genes([with_letters(g, b"Y", 40 + j) for j, g in enumerate(new)])))
    assert c == _lib.PDL_ERR_UNSUPPORTED and "0x59" in msg and "not in the base's alphabet: the union would rank k-mers differently" in msg
    nat.close()
    res, off, gen = _y_in_a_short_gene()
    nat = _native(4, res, off, gen)
    c, msg = _code(lambda: nat.remove([0]))
    assert c == _lib.PDL_ERR_UNSUPPORTED and "'Y'" in msg and "conservative" in msg
    with pytest.raises(_lib.PdlError):
        nat.set_option("alphabet_rekey", 2)
    nat.close()


# ---- 8. random sets: every seed equals the oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", list(range(REKEY_SEED0, REKEY_SEED0 + N_SEEDS)))
def test_random_sets_equal_the_oracle(seed):
    case = rekey_case(seed)
    assert classify_rekey(case) == "supported"
    k = case["k"]
    nat = _native(k, *case["base"], options=ON)
    if case["mode"] == "append":
        nat.append(*case["query"])
    else:
        nat.remove(case["removed"])
    target = case["target"]
    changed = len(np.unique(case["base"][0])) != len(np.unique(target[0]))
    assert nat.last_rekey_info["rekeyed"] == int(changed), f"seed {seed}"
    _assert_oracle(nat, *target, k, f"seed {seed} ({case['mode']})")
    _assert_dictionary_is_the_oracles(nat, *target, k, f"seed {seed}")
    nat.close()


# ---- 9. the commands ---------------------------------------------------------------------------------------------------------------------
def _records(label, genes, tag):
    return [(label, b"%s%d" % (tag, i), g) for i, g in enumerate(genes)]


def _write(path, recs):
    path.write_bytes(b"".join(b"%s\t%s\tp\n%s\n" % r for r in recs))


def test_commands_with_rekey_write_the_net_of_the_resulting_set(tmp_path, capsys):
    from pandelos_amd import append as A
    from pandelos_amd import pangenes as P
    from pandelos_amd import remove as R
    fam = family_genes(A19, 4, 8, 40, 70, 33, sub=0.05)
    recs = [r for g in range(3) for r in _records(b"G%d" % g, fam[g], b"g%d_" % g)]
    new = _records(b"G3", [with_letters(g, b"Y", 40 + j) for j, g in enumerate(fam[3])], b"n")
    base, more, union, net, want = (tmp_path / n for n in ("base.faa", "more.faa", "union.faa", "out.net", "want.net"))
    _write(base, recs); _write(more, new); _write(union, recs + new)
    assert A.main(["-i", str(base), "-k", "4", "-a", str(more), "--rekey", "-o", str(net)]) == 0
    assert "alphabet 19 -> 20 letters" in capsys.readouterr().out
    assert P.main(["-i", str(union), "-k", "4", "-o", str(want)]) == 0
    assert net.read_bytes() == want.read_bytes() and len(want.read_bytes()) > 0
    # ... and back: G3 leaves the union, the library re-keys instead of the command rebuilding
    assert R.main(["-i", str(union), "-k", "4", "-r", "G3", "--rekey", "-o", str(net)]) == 0
    out = capsys.readouterr().out
    assert "alphabet 20 -> 19 letters" in out and "rebuilding" not in out
    assert P.main(["-i", str(base), "-k", "4", "-o", str(want)]) == 0
    assert net.read_bytes() == want.read_bytes() and len(want.read_bytes()) > 0
