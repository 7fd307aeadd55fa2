"""pdl_remove_genomes without a GPU: the binding agrees with the header, both libraries export the symbol, the remove command
refuses what cannot be meant before any device call, `remaining_input` undoes the intruder construction the GPU tests pin
every fixture with, and the seed range of the GPU fuzz test is mostly usable."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "pandelos_amd" / "lib"
REMOVE_SEED0, REMOVE_SEEDS_DEFAULT = 9000, 120        # the range tests/test_gpu_remove.py runs by default
POSITIONS = ("front", "middle", "interleaved", "end")
MASK64 = (1 << 64) - 1
RABIN_MODULO = 18446744073709551557


# ---- the construction that lets every pinned set pin a removal -----------------------------------------------------------------
def intruder_genes(res, off, seed, count=7, like=None):
    """`count` genes over the letters of the set itself: random ones, and copies of genes of the set with a few letters
    changed (so that the intruder shares k-mers, groups and best hits with the set while it is in)."""
    rng = np.random.default_rng(seed)
    res = np.asarray(res, np.uint8)
    off = np.asarray(off).astype(np.int64)
    letters = np.unique(res)
    genes = []
    for j in range(count):
        if j % 2 == 0 and len(off) > 1:
            i = int(rng.integers(0, len(off) - 1))
            g = res[off[i]:off[i + 1]].copy()
            m = rng.random(len(g)) < 0.08
            g[m] = letters[rng.integers(0, len(letters), int(m.sum()))]
        else:
            g = letters[rng.integers(0, len(letters), int(rng.integers(1, like or 120)))]
        genes.append(g.astype(np.uint8))
    return genes


def splice(res, off, gen, genes, position):
    """The set with the intruder's genes in it -> (residues, offsets, genome_of, intruder's genome id).  Genome ids are dense in
    first-seen order, as PangeneIData assigns them: an intruder at the front is genome 0 and every other genome moves up."""
    res = np.asarray(res, np.uint8)
    off = np.asarray(off).astype(np.int64)
    own = [(res[off[i]:off[i + 1]], int(gen[i])) for i in range(len(gen))]
    new = [(g, -1) for g in genes]
    if position == "front":
        seq = new + own
    elif position == "end":
        seq = own + new
    elif position == "middle":
        h = len(own) // 2
        seq = own[:h] + new + own[h:]
    elif position == "interleaved":
        seq, a, b = [], list(own), list(new)
        while a or b:
            if a:
                seq.append(a.pop(0))
            if b:
                seq.append(b.pop(0))
    else:
        raise ValueError(position)
    ids, out_gen = {}, []
    for _, lab in seq:
        out_gen.append(ids.setdefault(lab, len(ids)))
    o = np.zeros(len(seq) + 1, np.uint64)
    np.cumsum([len(g) for g, _ in seq], out=o[1:])
    r = np.concatenate([g for g, _ in seq]).astype(np.uint8) if seq else np.zeros(0, np.uint8)
    return r, o, np.asarray(out_gen, np.uint32), ids[-1]


# ---- what the library must answer, from the inputs alone --------------------------------------------------------------------------
def rank_init_overflows(base, k):
    """rank_init's own overflow test (library.cpp:101-119: wrapped 64-bit products, one multiplication ahead)."""
    lm, over = 1, False
    for _ in range(k - 1):
        t = lm
        lm = (lm * base) & MASK64
        if over:
            lm %= RABIN_MODULO
        elif t > lm or ((t * base) & MASK64) > ((lm * base) & MASK64):
            over = True
            lm = ((t % RABIN_MODULO) * base) % RABIN_MODULO
    return over


def classify_removal(res, off, gen, k, removed):
    """'skip' (one genome only: nothing can be removed), 'undecodable' / 'alphabet' (PDL_ERR_UNSUPPORTED), 'empty'
    (PDL_ERR_EMPTY) or 'ok' — in the order the library checks."""
    res = np.asarray(res, np.uint8)
    off = np.asarray(off).astype(np.int64)
    gen = np.asarray(gen)
    if len(gen) == 0 or int(gen.max()) == 0:
        return "skip"
    lens = np.diff(off)
    if int(np.maximum(lens - k + 1, 0).sum()) == 0:
        return "empty"                                  # (the set itself has no k-mer: pdl_preprocess says so, and nothing can be removed)
    base = len(np.unique(res)) & 0xff                   # (rank_base is an unsigned char)
    if base == 0 or rank_init_overflows(base, k) or base ** k >= 1 << 64:
        return "undecodable"
    stays = ~np.isin(gen, list(removed))
    long_enough = stays & (lens >= k)
    if not long_enough.any():
        return "empty"
    seen = np.zeros(256, bool)
    for i in np.nonzero(long_enough)[0]:
        seen[res[off[i]:off[i + 1]]] = True
    return "ok" if seen.sum() == len(np.unique(res)) else "alphabet"


def fuzz_case(seed):
    """-> (residues, offsets, genome_of, k, removed genome ids, verdict) of one fuzz seed"""
    from tests.test_gpu_fuzz import _random_set
    res, off, gen, k = _random_set(seed)
    G = int(gen.max()) + 1 if len(gen) else 0
    if G < 2:
        return res, off, gen, k, [], "skip"
    rng = np.random.default_rng(seed ^ 0x5eed)
    r = int(rng.integers(1, G))
    removed = sorted(int(x) for x in rng.choice(G, r, replace=False))
    return res, off, gen, k, removed, classify_removal(res, off, gen, k, removed)


# ---- 1. the binding ------------------------------------------------------------------------------------------------------------
def test_remove_info_matches_the_header(tmp_path):
    from pandelos_amd import _lib
    src, exe = tmp_path / "size.c", tmp_path / "size"
    src.write_text('#include <stdio.h>\n#include "pandelos_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(pdl_remove_info), offsetof(pdl_remove_info, residues), '
                   'offsetof(pdl_remove_info, records), offsetof(pdl_remove_info, compact_ms), offsetof(pdl_remove_info, device_ms)); return 0; }\n')
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    size, o_res, o_rec, o_cmp, o_dev = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    I = _lib.PdlRemoveInfo
    assert C.sizeof(I) == size
    assert (I.sequences.offset, I.residues.offset, I.records.offset, I.compact_ms.offset, I.device_ms.offset) == (0, o_res, o_rec, o_cmp, o_dev)
    assert "pdl_remove_genomes" in _lib.EXPORTS


@pytest.mark.parametrize("lib", ["libpandelos_amd.so", "libnative.so"])
def test_libraries_export_the_symbol(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB / lib)], check=True, capture_output=True, text=True).stdout
    assert any(line.split()[-1] == "pdl_remove_genomes" for line in out.splitlines() if line.strip())


# ---- 2. the command --------------------------------------------------------------------------------------------------------------
def _write(path, recs):
    path.write_bytes(b"".join(b"%s\t%s\tp\n%s\n" % r for r in recs))


def test_remove_command_refuses_bad_labels_before_the_device_is_touched(tmp_path, capsys, monkeypatch):
    from pandelos_amd import pangene_native
    from pandelos_amd import remove as R
    base, new = tmp_path / "base.faa", tmp_path / "new.faa"
    _write(base, [(b"A", b"a1", b"ACDEFG"), (b"B", b"b1", b"CDEFGH"), (b"A", b"a2", b"ACDEFH")])
    _write(new, [(b"A", b"x1", b"ACDEFG")])

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the labels were checked")
    monkeypatch.setattr(pangene_native.PangeneNative, "open", staticmethod(no_device))
    out = tmp_path / "rest.net"
    common = ["-i", str(base), "-k", "3", "-o", str(out)]
    assert R.main(common + ["-r", "Z"]) == 2
    assert "'Z' names no genome" in capsys.readouterr().err
    assert R.main(common + ["-r", "A", "-r", "B"]) == 2
    assert "nothing would remain" in capsys.readouterr().err
    assert R.main(common) == 2
    assert "no genome to remove" in capsys.readouterr().err
    assert R.main(common + ["-r", "B", "-r", "B"]) == 2
    assert "named twice" in capsys.readouterr().err
    # a label that stays clashes with an appended file; the one that leaves is free again
    assert R.main(common + ["-r", "B", "-a", str(new)]) == 2
    assert "'A' already names a genome" in capsys.readouterr().err
    assert not out.exists()
    assert R.check_remove(["B"], ["A", "B"]) == [1]
    with pytest.raises(AssertionError, match="device was touched"):
        R.main(common + ["-r", "A", "-a", str(new)])


# ---- 3. remaining_input undoes the intruder ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("position", POSITIONS)
@pytest.mark.parametrize("case", ["readme4_k2", "interleaved_genomes", "synth_5x60x80_k3"])
def test_remaining_input_undoes_the_intruder(case, position):
    from pandelos_amd.remove import remaining_input
    from tests import helpers as H
    res, off, gen, k, _ = H.load_small(case)
    r2, o2, g2, gx = splice(res, off, gen, intruder_genes(res, off, 5), position)
    assert len(g2) == len(gen) + 7 and int(g2.max()) == int(gen.max()) + 1
    assert gx == {"front": 0, "end": int(gen.max()) + 1}.get(position, gx)
    r3, o3, g3 = remaining_input(r2, o2, g2, [gx])
    assert r3.tobytes() == np.asarray(res, np.uint8).tobytes()
    assert o3.dtype == np.uint64 and np.array_equal(o3, np.asarray(off, np.uint64))
    assert g3.dtype == np.uint32 and np.array_equal(g3, np.asarray(gen, np.uint32))


def test_remaining_input_agrees_with_the_split_of_the_query_tests():
    from pandelos_amd.remove import remaining_input
    from pandelos_amd.synth import make_gene_set
    from tests.test_gpu_query import _split
    gs = make_gene_set(genomes=5, genes_per_genome=20, mean_len=50, sub_rate=0.1, seed=3)
    last = int(gs.genome_of.max())
    (rb, ob_, gb), _ = _split(gs.residues, gs.offsets, gs.genome_of, last)
    r3, o3, g3 = remaining_input(gs.residues, gs.offsets, gs.genome_of, [last])
    assert r3.tobytes() == rb.tobytes() and np.array_equal(o3, ob_) and np.array_equal(g3, gb)
    # ... and for a genome in the middle of a set whose genomes are interleaved
    r2, o2, g2, gx = splice(gs.residues, gs.offsets, gs.genome_of, intruder_genes(gs.residues, gs.offsets, 9), "interleaved")
    (rb, ob_, gb), _ = _split(r2, o2, g2, gx)
    r3, o3, g3 = remaining_input(r2, o2, g2, [gx])
    assert r3.tobytes() == rb.tobytes() and np.array_equal(o3, ob_) and np.array_equal(g3, gb)


# ---- 4. the fuzz range -------------------------------------------------------------------------------------------------------------
def test_the_fuzz_seed_range_is_mostly_usable():
    """tests/test_gpu_remove.py skips the seeds that give nothing to remove from; every other seed is a test case, the ones the
    library must refuse included.  At most a quarter of the default range may be skipped."""
    verdicts = [fuzz_case(seed)[5] for seed in range(REMOVE_SEED0, REMOVE_SEED0 + REMOVE_SEEDS_DEFAULT)]
    count = {v: verdicts.count(v) for v in ("ok", "skip", "undecodable", "alphabet", "empty")}
    print(count)
    assert sum(count.values()) == REMOVE_SEEDS_DEFAULT
    assert 4 * count["skip"] <= REMOVE_SEEDS_DEFAULT, count
    assert count["ok"] >= REMOVE_SEEDS_DEFAULT // 2 and count["undecodable"] and count["alphabet"] and count["empty"], count
