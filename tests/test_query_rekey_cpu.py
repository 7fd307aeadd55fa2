"""Option "query_rekey" without a GPU: the reference-pinned fixtures of tests/golden/query_rekey through the CPU oracle (and the
reference build where it exists); the model of Q-rebase on every key of every fixture's union dictionary and at the edges of its
arithmetic; the generator of the GPU test's random cases, as a condition; the four commands' flag; the binding of
pdl_query_rekey_info."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import query_rekey_sets as S
from tests.test_query_golden import assert_block, union_arrays
from tests.test_rekey_cpu import rank_table

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "pandelos_amd" / "lib"


def test_the_fixture_set_is_complete_and_small():
    assert len(S.CASES) == 6, S.CASES
    largest = max(p.stat().st_size for p in (S.QRDIR.parent / "query").glob("*.npz"))
    assert all((S.QRDIR / f"{name}.npz").stat().st_size <= largest for name in S.CASES)


@pytest.mark.parametrize("name", S.CASES)
def test_fixture_reproduces_through_the_oracle_on_the_union(name):
    from oracle import binding as ob
    fx, base, query, k, G = S.load_case(name)
    res, off, gen, g_union = union_arrays(base, query)
    assert g_union == G
    assert set(query.flatten()[0].tolist()) - set(base.flatten()[0].tolist()), "the query brings no letter"
    ora = ob.Oracle(res, off, gen, k)
    assert ora.genomes == G + 1 and not ora.hash_fallback
    assert_block(ora.scores(G), fx, name)
    assert ora.genome_cost(G) == int(fx["genome_cost"])


@pytest.mark.parametrize("name", S.CASES)
def test_fixture_reproduces_through_the_reference_build(name, tmp_path):
    from oracle import binding as ob
    if not ob.have_reference():
        pytest.skip("no reference build in oracle/_ref")
    fx, _, _, k, G = S.load_case(name)
    union = tmp_path / "union.faa"
    union.write_bytes(fx["base_faa"].tobytes() + fx["query_faa"].tobytes())
    info = ob.run_harness(ob.REF_SO, union, k, dump=tmp_path / "out.bin")
    ref = ob.read_dump(tmp_path / "out.bin")
    assert ref["genomes"] == G + 1
    assert_block(ref["per_genome"][G], fx, name)
    assert info["genome_cost"][G] == int(fx["genome_cost"])


def test_the_fold_shapes_are_what_the_names_say():
    from tests.golden.make_golden_query_rekey import fold_shape, make_cases
    for name, (base, q, k, shape, letters) in make_cases().items():
        assert name in S.CASES
        assert set(b"".join(q)) - set(b"".join(s for _, s in base)) == set(letters), name
        if shape is not None:
            assert fold_shape([s for _, s in base], q, k) == shape, name
    short = make_cases()["new_letter_only_in_a_short_gene"]
    assert all(b"A" not in g for g in short[1] if len(g) >= short[2]) and any(b"A" in g for g in short[1])


# ---- the model of Q-rebase ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.CASES)
def test_rebase_model_on_every_key_of_the_unions_dictionary(name):
    """A union key without a new letter, written back, is the base's key of the same k-mer; one with a new letter is flagged.  The
    k-mer of a key is known here: the union's dictionary is walked gene by gene."""
    from oracle import binding as ob
    fx, base, query, k, G = S.load_case(name)
    res, off, gen, _ = union_arrays(base, query)
    base_letters, union_letters = bytes(sorted(set(base.flatten()[0].tolist()))), bytes(sorted(set(res.tolist())))
    tb, tu = rank_table(base_letters), rank_table(union_letters)
    plan = S.rebase_plan(base_letters, union_letters, k)
    ranks = set(int(r) for r in ob.Oracle(res, off, gen, k).dictionary()["rank"])
    seen, flagged = set(), 0
    off = off.astype(np.int64)
    for i in range(len(gen)):
        g = res[off[i]:off[i + 1]].tobytes()
        for j in range(len(g) - k + 1):
            kmer = g[j:j + k]
            x = S.key_of(kmer, tu, len(tu))
            assert x in ranks
            seen.add(x)
            y, none = S.rebase_one(x, plan)
            has_new = any(b not in tb for b in kmer)
            assert none == has_new, (name, kmer)
            if not has_new:
                assert y == S.key_of(kmer, tb, len(tb)), (name, kmer)
            flagged += has_new
    assert seen == ranks
    if name != "new_letter_only_in_a_short_gene":
        assert flagged > 0, name
    else:
        assert flagged == 0


def test_rebase_model_at_the_edges_of_one_two_and_three_parts():
    """B' = 2, 5, 21, 25 at k that cut a key into one, two and — where B'^(2h + 1) still fits 64 bits: 5 and 25 — three parts:
    the smallest and largest keys, keys around every multiple of B'^h, keys with and without a new letter."""
    for B2, ks in [(2, ((20, 1), (40, 2), (63, 2))), (5, ((13, 1), (26, 2), (27, 3))), (21, ((7, 1), (14, 2))), (25, ((6, 1), (12, 2), (13, 3)))]:
        union = bytes(range(65, 65 + B2))
        for k, parts in ks:
            for new in ({union[0]}, {union[-1]}, {union[B2 // 2]}, {union[0], union[-1]} if B2 > 2 else {union[0]}):
                base = bytes(b for b in union if b not in new)
                plan = S.rebase_plan(base, union, k)
                assert plan["nparts"] == parts, (B2, k, plan["nparts"])
                tb, tu = rank_table(base), rank_table(union)
                top, div = B2 ** k, plan["part_div"]
                xs = {0, 1, top - 1, top // 2, div - 1, div, div + 1, top - div, top - div - 1}
                for mult in (1, 2, B2 - 1, B2):
                    for delta in (-1, 0, 1):
                        xs.update({mult * div * div + delta, mult * div + delta})
                rng = np.random.default_rng(B2 * 1000 + k)
                xs.update(int(x) % top for x in rng.integers(0, 1 << 63, 100, dtype=np.uint64))
                # keys spelt with base letters only, among them the largest such key
                for _ in range(50):
                    xs.add(S.key_of(bytes(base[int(i)] for i in rng.integers(0, len(base), k)), tu, B2))
                xs.add(S.key_of(bytes([base[-1]]) * k, tu, B2))
                inv = {d: b for b, d in tu.items()}
                for x in xs:
                    if not 0 <= x < top:
                        continue
                    kmer, rest = [], x
                    for _ in range(k):
                        kmer.append(inv[rest % B2])
                        rest //= B2
                    kmer = bytes(reversed(kmer))
                    y, none = S.rebase_one(x, plan)
                    assert none == any(b in new for b in kmer), (B2, k, x)
                    if not none:
                        assert y == S.key_of(kmer, tb, len(tb)) and y < len(tb) ** k, (B2, k, x)


# ---- the random cases of the GPU test -------------------------------------------------------------------------------------------------
def test_every_default_seed_is_supported_and_the_construction_places_the_letter():
    for seed in range(S.SEED0, S.SEED0 + S.SEEDS_DEFAULT):
        case = S.query_rekey_case(seed)
        assert S.classify(case) == "supported", seed
        base_letters, query_letters = set(case["base"][0].tolist()), set(case["query"][0].tolist())
        new = query_letters - base_letters
        assert len(base_letters | query_letters) <= 12 and case["k"] <= 8, seed
        assert base_letters == set(case["alphabet"]) and new == set(case["letters"] + case["short_letter"]) and new, seed
        lo, hi, k = min(base_letters), max(base_letters), case["k"]
        in_kmers = set(b"".join(g for g in case["query_genes"] if len(g) >= k)) - base_letters
        assert in_kmers == set(case["letters"]), seed
        where = ("below", "between", "above", "two")[seed % 4]
        assert case["where"] == where
        if where == "below":
            assert all(b < lo for b in in_kmers), seed
        elif where == "above":
            assert all(b > hi for b in in_kmers), seed
        elif where == "between":
            assert all(lo < b < hi for b in in_kmers), seed
        else:
            assert len(in_kmers) == 2 and sum(lo < b < hi for b in in_kmers) == 1, seed
        if seed % 8 >= 4:
            only_short = new - in_kmers
            assert only_short == set(case["short_letter"]) and only_short, seed
            assert any(len(g) < k and set(g) & only_short for g in case["query_genes"]), seed
        else:
            assert not case["short_letter"], seed


# ---- the commands and the binding -----------------------------------------------------------------------------------------------------
def test_the_four_commands_take_the_flag_and_check_labels_first(tmp_path, capsys, monkeypatch):
    from pandelos_amd import pangene_native
    from pandelos_amd import place as P
    from pandelos_amd import place_batch as PB
    from pandelos_amd import query as Q
    from pandelos_amd import query_batch as QB
    base, clash = tmp_path / "base.faa", tmp_path / "clash.faa"
    base.write_bytes(b"A\ta1\tp\nACDEFG\nB\tb1\tp\nCDEFGH\n")
    clash.write_bytes(b"B\tq1\tp\nACDEFX\n")

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the labels were checked")
    monkeypatch.setattr(pangene_native.PangeneNative, "open", staticmethod(no_device))
    common = ["-i", str(base), "-k", "3", "-q", str(clash), "--rekey"]
    for main, rest in ((Q.main, ["-o", str(tmp_path / "o.net")]), (P.main, ["-o", str(tmp_path / "o.tsv")]),
                       (QB.main, ["--out-dir", str(tmp_path / "qb")]), (PB.main, ["--out-dir", str(tmp_path / "pb")])):
        assert main(common + rest) == 2
        assert "already names a base genome" in capsys.readouterr().err


def test_query_rekey_info_matches_the_header(tmp_path):
    from pandelos_amd import _lib
    fields = [n for n, _ in _lib.PdlQueryRekeyInfo._fields_]
    assert fields == ["queries_rekeyed", "letters_base", "letters_max", "key_bits_base", "key_bits_max", "records_rebased", "rebase_ms"]
    src, exe = tmp_path / "size.c", tmp_path / "size"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pandelos_amd.h"\nint main(void) { printf("%zu", sizeof(pdl_query_rekey_info));\n'
                   + "".join(f'printf(" %zu", offsetof(pdl_query_rekey_info, {n}));\n' for n in fields) + "return 0; }\n")
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    size, *offs = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert C.sizeof(_lib.PdlQueryRekeyInfo) == size
    assert [getattr(_lib.PdlQueryRekeyInfo, n).offset for n in fields] == offs
    assert "pdl_get_query_rekey_info" in _lib.EXPORTS


@pytest.mark.parametrize("lib", ["libpandelos_amd.so", "libnative.so"])
def test_libraries_export_the_getter(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB / lib)], check=True, capture_output=True, text=True).stdout
    assert any(line.split()[-1] == "pdl_get_query_rekey_info" for line in out.splitlines() if line.strip())
