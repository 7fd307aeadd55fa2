"""K-rekey without a GPU: a model of the re-key pass in Python integers — the arithmetic of pdl_rekey.h, plan and kernel, step
for step — checked against the CPU oracle's dictionaries where an alphabet grows or shrinks; the binding of pdl_rekey_info; the
set builder, the case generator and the classifier of tests/test_gpu_rekey.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "pandelos_amd" / "lib"
REKEY_SEED0, REKEY_SEEDS_DEFAULT = 12000, 60          # the range tests/test_gpu_rekey.py runs by default
MASK64 = (1 << 64) - 1


# ---- the model: pdl_rekey.h in Python integers ------------------------------------------------------------------------------------
def rank_table(letters):
    """rank_values of an alphabet (library.cpp:96-99): dense digits in byte order -> {byte: digit}"""
    return {b: d for d, b in enumerate(sorted(set(int(x) for x in letters)))}


def rekey_plan(old_letters, new_letters, k):
    """rk_plan: the kernel's arguments and its table T[i][d] = map[d] * B'^i."""
    old, new = rank_table(old_letters), rank_table(new_letters)
    B, B2 = len(old), len(new)
    assert B >= 1 and B ** k < 1 << 64 and B2 ** k < 1 << 64
    h, div = 0, 1
    while h < k and div * B <= 1 << 32:
        div *= B
        h += 1
    plan = dict(k=k, base=B, h=h, nparts=(k + h - 1) // h, part_div=div,
                magic=(MASK64 // B + 1) & MASK64 if B > 1 else 0,
                part_magic=(MASK64 // div + (1 if MASK64 % div == div - 1 else 0)) if div > 1 else 0)
    table = [0] * (k * B)
    for i in range(k):
        for b, d in old.items():
            if b in new:
                table[i * B + d] = new[b] * B2 ** i
    plan["table"] = table
    return plan


def rekey_one(x, plan, key64_in):
    """rk_items for one key: parts by a multiply-high with floor(2^64 / B^h) and one correction, digits by one multiplication."""
    k, B, h = plan["k"], plan["base"], plan["h"]
    rest, left, row, y = int(x), k, 0, 0
    for p in range(plan["nparts"]):
        nd = min(left, h)
        if key64_in and p + 1 < plan["nparts"]:
            q = (rest * plan["part_magic"]) >> 64
            r = rest - q * plan["part_div"]
            assert 0 <= r < 2 * plan["part_div"]                     # the estimate is the quotient or one below it
            if r >= plan["part_div"]:
                q, r = q + 1, r - plan["part_div"]
            part, rest = r, q
        else:
            part = rest
        assert part < 1 << 32
        for _ in range(nd):
            q = (part * plan["magic"]) >> 64
            d = part - q * B
            assert 0 <= d < B and (B == 1 or q == part // B)
            y += plan["table"][row + d]
            part, row = q, row + B
        left -= nd
    assert y < 1 << 64
    return y


def rekey_ranks(ranks, old_letters, new_letters, k):
    plan = rekey_plan(old_letters, new_letters, k)
    key64 = len(rank_table(old_letters)) ** k > 1 << 32
    return np.array([rekey_one(int(x), plan, key64) for x in ranks], np.uint64)


# ---- small sets of related genomes over a chosen alphabet -------------------------------------------------------------------------
def pack(seqs, genome_of):
    res = np.frombuffer(b"".join(bytes(s) for s in seqs), np.uint8).copy()
    off = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(x) for x in seqs], out=off[1:])
    return res, off, np.asarray(genome_of, np.uint32)


def family_genes(alphabet, genomes, genes, lo, hi, seed, sub=0.1):
    """`genomes` lists of `genes` genes each: mutated copies (substitutions inside `alphabet`) of one random ancestor genome with
    genes of lo..hi residues — related enough to share k-mers, score and form edges."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(bytes(alphabet), np.uint8)
    anc = [alpha[rng.integers(0, len(alpha), int(rng.integers(lo, hi + 1)))] for _ in range(genes)]
    out = []
    for _ in range(genomes):
        gs = []
        for a in anc:
            g = a.copy()
            m = rng.random(len(g)) < sub
            g[m] = alpha[rng.integers(0, len(alpha), int(m.sum()))]
            gs.append(g.tobytes())
        out.append(gs)
    return out


def with_letters(gene, letters, seed, every=9):
    """`gene` with about one residue in `every` replaced by one of `letters`."""
    rng = np.random.default_rng(seed)
    g = np.frombuffer(gene, np.uint8).copy()
    m = rng.random(len(g)) < 1.0 / every
    if len(g) and not m.any():
        m[int(rng.integers(0, len(g)))] = True
    ls = np.frombuffer(bytes(letters), np.uint8)
    g[m] = ls[rng.integers(0, len(ls), int(m.sum()))]
    return g.tobytes()


def kmers(off, k):
    return int(np.maximum(np.diff(np.asarray(off).astype(np.int64)) - k + 1, 0).sum())


# ---- 1. the model against the oracle's dictionaries -----------------------------------------------------------------------------------
GROWTH = [(b"ACGT", b"N", 16), (b"ACDEFGHIKLMNPQRSTVWY", b"XU", 5), (b"CDEF", b"A", 3), (b"CDEF", b"Z", 3), (b"BD", b"ACE", 7), (b"A", b"C", 4)]


def _growth_sets(old, add, k, seed):
    fam = family_genes(old, 3, 6, k, k + 40, seed)
    base = pack([g for gs in fam for g in gs], [i for i, gs in enumerate(fam) for _ in gs])
    new = [with_letters(g, add, seed + j) for j, g in enumerate(family_genes(old, 1, 6, k, k + 40, seed)[0])]
    new[0] = new[0][:k - 1] + bytes(add)                            # every new letter at least once (here: in a gene of k + ... residues)
    return base, new


@pytest.mark.parametrize("old,add,k", GROWTH)
def test_rekeyed_base_dictionary_is_the_base_part_of_the_unions(old, add, k):
    from oracle import binding as ob
    (res, off, gen), new = _growth_sets(old, add, k, 31 * k + len(add))
    nb = len(gen)
    ures, uoff, ugen = pack([res[int(off[i]):int(off[i + 1])].tobytes() for i in range(nb)] + new, list(gen) + [int(gen.max()) + 1] * len(new))
    assert set(np.unique(ures)) == set(old + add)
    base, union = ob.Oracle(res, off, gen, k), ob.Oracle(ures, uoff, ugen, k)
    assert not base.hash_fallback and not union.hash_fallback
    db, du = base.dictionary(), union.dictionary()
    du = du[du["seq"] < nb]                                         # the base genes' records of the union's dictionary, in its order
    got = rekey_ranks(db["rank"], old, old + add, k)
    assert len(db) == len(du) and len(db) > 0
    assert np.array_equal(got, du["rank"]) and np.array_equal(db["seq"], du["seq"]) and np.array_equal(db["count"], du["count"])
    # ... and back: the union's keys that hold no new letter, written for the smaller alphabet, are the base's
    back = rekey_ranks(du["rank"], old + add, old, k)
    assert np.array_equal(back, db["rank"])


def test_model_divides_exactly_at_the_edges_of_every_base():
    """The two reciprocals at the values where a rounded one would fail first: around every multiple of B^h and of B near 2^32
    and 2^64 (rekey_one asserts every quotient)."""
    for B, k in [(2, 63), (3, 40), (4, 31), (5, 27), (7, 22), (16, 15), (20, 14), (21, 14), (23, 14), (84, 10), (138, 9), (255, 8), (256, 7)]:
        letters = bytes(range(B))
        plan = rekey_plan(letters, letters, k)                      # the identity: decoding and encoding must give the key back
        top = B ** k
        xs = {0, 1, top - 1, top // 2, plan["part_div"] - 1, plan["part_div"], plan["part_div"] + 1}
        for mult in (1, 2, 3, B - 1, B, B + 1):
            for delta in (-1, 0, 1):
                xs.add(mult * plan["part_div"] ** 2 + delta)
                xs.add(top - mult * plan["part_div"] + delta)
        rng = np.random.default_rng(B * 100 + k)
        xs.update(int(x) % top for x in rng.integers(0, 1 << 63, 200, dtype=np.uint64))
        for x in xs:
            if 0 <= x < top:
                assert rekey_one(x, plan, top > 1 << 32) == x, (B, k, x)


# ---- 2. the binding ---------------------------------------------------------------------------------------------------------------
def test_rekey_info_matches_the_header(tmp_path):
    from pandelos_amd import _lib
    fields = [n for n, _ in _lib.PdlRekeyInfo._fields_]
    src, exe = tmp_path / "size.c", tmp_path / "size"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pandelos_amd.h"\nint main(void) { printf("%zu", sizeof(pdl_rekey_info));\n'
                   + "".join(f'printf(" %zu", offsetof(pdl_rekey_info, {n}));\n' for n in fields) + "return 0; }\n")
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    size, *offs = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert C.sizeof(_lib.PdlRekeyInfo) == size
    assert [getattr(_lib.PdlRekeyInfo, n).offset for n in fields] == offs
    assert "pdl_get_rekey_info" in _lib.EXPORTS


@pytest.mark.parametrize("lib", ["libpandelos_amd.so", "libnative.so"])
def test_libraries_export_the_getter(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB / lib)], check=True, capture_output=True, text=True).stdout
    assert any(line.split()[-1] == "pdl_get_rekey_info" for line in out.splitlines() if line.strip())


def test_commands_take_the_flag_and_check_labels_first(tmp_path, capsys, monkeypatch):
    from pandelos_amd import append as A
    from pandelos_amd import pangene_native
    from pandelos_amd import remove as R
    base = tmp_path / "base.faa"
    base.write_bytes(b"A\ta1\tp\nACDEFG\nB\tb1\tp\nCDEFGH\n")

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the labels were checked")
    monkeypatch.setattr(pangene_native.PangeneNative, "open", staticmethod(no_device))
    assert R.main(["-i", str(base), "-k", "3", "-o", str(tmp_path / "o.net"), "--rekey", "-r", "Z"]) == 2
    assert "'Z' names no genome" in capsys.readouterr().err
    assert A.main(["-i", str(base), "-k", "3", "-o", str(tmp_path / "o.net"), "--rekey", "-a", str(base)]) == 2
    assert "already names a genome" in capsys.readouterr().err


# ---- 3. the random cases of the GPU test ------------------------------------------------------------------------------------------------
POOL = b"#*ABCDEFGHIKLMNPQRSTVWXYZ"                    # two bytes below 'A' among them


def rekey_case(seed):
    """-> dict(mode 'append' | 'remove', k, whole set (res, off, gen), base (res, off, gen), query (res, off) or None,
    removed ids or None, target set (res, off, gen)).  Alphabets of at most 12 letters, k <= 8: B^k is always exact.  Every genome
    draws its own sub-alphabet and holds at least one gene of k residues or more, and a few shorter ones."""
    from pandelos_amd.remove import remaining_input
    rng = np.random.default_rng(seed)
    pool = np.frombuffer(POOL, np.uint8)
    sup = np.sort(rng.choice(pool, int(rng.integers(2, 13)), replace=False))
    k = int(rng.integers(2, 9))
    G = int(rng.integers(3, 7))
    # one genome (the appended one; any one of a removal) spells with the whole alphabet, the others with a part of it
    core = np.sort(rng.choice(sup, int(rng.integers(1, len(sup) + 1)), replace=False))
    special = G - 1 if seed % 2 == 0 else int(rng.integers(0, G))
    anc = [sup[rng.integers(0, len(sup), int(rng.integers(k, 70)))] for _ in range(int(rng.integers(3, 9)))]
    seqs, gen = [], []
    for g in range(G):
        mine = sup if g == special else core
        own = np.sort(rng.choice(mine, int(rng.integers(1, len(mine) + 1)), replace=False))
        for a in anc:
            x = own[np.searchsorted(own, a) % len(own)].copy()       # the ancestor's gene, spelt with the genome's letters
            m = rng.random(len(x)) < 0.1
            x[m] = own[rng.integers(0, len(own), int(m.sum()))]
            seqs.append(x.tobytes()); gen.append(g)
        for _ in range(int(rng.integers(0, 4))):                     # genes shorter than k: letters that may show in no key
            seqs.append(mine[rng.integers(0, len(mine), int(rng.integers(0, k)))].tobytes()); gen.append(g)
    res, off, gen = pack(seqs, gen)
    case = dict(k=k, whole=(res, off, gen), query=None, removed=None)
    if seed % 2 == 0:
        case["mode"] = "append"
        n = int((gen < G - 1).sum())
        cut = int(off[n])
        case["base"] = (res[:cut].copy(), off[:n + 1].copy(), gen[:n].copy())
        case["query"] = (res[cut:].copy(), (off[n:] - off[n]).astype(np.uint64))
        case["target"] = (res, off, gen)
    else:
        case["mode"] = "remove"
        removed = set(int(x) for x in rng.choice(G, int(rng.integers(1, G)), replace=False))
        if rng.random() < 0.7 and len(removed | {special}) < G:
            removed.add(special)
        removed = sorted(removed)
        case["base"], case["removed"] = (res, off, gen), removed
        case["target"] = remaining_input(res, off, gen, removed)
    return case


def classify_rekey(case):
    """What the library must answer, from the inputs alone: 'supported', or the refusal ('empty', 'inexact')."""
    k = case["k"]
    for res, off, _ in (case["base"], case["target"]):
        if kmers(off, k) == 0:
            return "empty"
        if len(np.unique(res)) ** k >= 1 << 64:
            return "inexact"
    return "supported"


def test_every_default_seed_is_supported_and_both_modes_move_the_alphabet():
    moved = {"append": 0, "remove": 0}
    short_only = 0
    for seed in range(REKEY_SEED0, REKEY_SEED0 + REKEY_SEEDS_DEFAULT):
        case = rekey_case(seed)
        assert classify_rekey(case) == "supported", seed
        a, b = set(np.unique(case["base"][0])), set(np.unique(case["target"][0]))
        assert len(a) <= 12 and len(b) <= 12 and case["k"] <= 8
        assert (a <= b) if case["mode"] == "append" else (b <= a)
        moved[case["mode"]] += a != b
        if case["mode"] == "remove" and a == b:
            res, off, _ = case["target"]
            lens = np.diff(off.astype(np.int64))
            in_kmers = set(np.unique(np.concatenate([res[int(off[i]):int(off[i + 1])] for i in np.nonzero(lens >= case["k"])[0]])))
            short_only += in_kmers != b
    print(moved, short_only)
    assert moved["append"] >= 5 and moved["remove"] >= 5, moved
