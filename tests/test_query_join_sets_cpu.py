"""tests/query_join_sets.py against itself, the source and the CPU oracle (no device): the module's constants are the kernels', every
case is what its plan says — recomputed from the oracle's dictionary and block of the union — and holds the numbers it was built
for, the rows that may leave the LDS table are stated as an interval, the table sequence's expectations follow from the host's
bookkeeping, and the read-out's struct is the header's."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import helpers as H
from tests import query_join_sets as S

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "pandelos_amd" / "csrc"
PLAN_FIELDS = ("records", "groups", "lookups", "chunk_lookups", "columns", "cells")


def _constant(text, name):
    return re.search(r"constexpr \w+ (?:\w+ = [^,;]+, )*" + name + r" = ([^,;]+)[,;]", text).group(1).strip()


def test_the_constants_are_the_kernels():
    text = (CSRC / "pdl_query.h").read_text()
    for name, value in S.SOURCE_CONSTANTS.items():
        assert int(_constant(text, name)) == value, name
    assert _constant(text, "QJ_HT") == "1u << QJ_HT_BITS" and S.QJ_HT == 1 << S.QJ_HT_BITS, "QJ_HT"
    assert _constant(text, "QJ_LIMIT") == "QJ_HT - 2 * QJ_T" and S.QJ_LIMIT == S.QJ_HT - 2 * S.QJ_T == 3584, "QJ_LIMIT"
    # the limit is read before the atomicCAS, by up to QJ_T threads at once: MUST_LEAVE rests on this line
    assert re.search(r"if \(\*\(volatile uint32_t \*\) &s_nkeys >= QJ_LIMIT\) return false;\s*\n\s*const uint32_t old = atomicCAS", text)
    # the prefilter holds a row's lookups against the same limit, in the single query and in the batch
    assert re.search(r"row_lookups\[g\] > limit", text) and text.count("QJ_LIMIT, qctl + Q_QRY_BOUND") == 1
    assert "QJ_LIMIT, w.rowid" in (CSRC / "pdl_query_batch.h").read_text()
    # the guard in front of the accumulator's 21-bit fields, at both doors
    assert f"<< {S.FIELD_BITS})" in text and "<< 42)" in text
    for t in (text, (CSRC / "pdl_query_batch.h").read_text()):
        assert t.count("(1u << 20)") + t.count("(1ull << 20)") >= 2 and S.GENE_KMERS_GUARD == 1 << 20


@pytest.fixture(scope="module")
def oracle_numbers():
    """per (case, query): what the oracle says about the query's rows; made once"""
    from oracle import binding as ob
    memo = {}

    def get(name, q):
        if (name, q) not in memo:
            c = S.case(name)
            res, off, gen, G = c.union(q)
            ora = ob.Oracle(res, off, gen, S.K)
            assert ora.genomes == G + 1 and ora.sequences == c.N + len(c.queries[q])
            memo[(name, q)] = S.from_oracle(ora.dictionary(), ora.scores(G), c.N, len(c.queries[q]))
            ora.close()
        return memo[(name, q)]
    return get


@pytest.mark.parametrize("name", S.all_names())
def test_every_case_is_what_its_plan_says(name, oracle_numbers):
    c = S.case(name)
    assert c.N < 20000 and all(len(q) <= len(S.SEPARATORS) for q in c.queries)
    seen = set()
    for q in range(len(c.queries)):
        key = repr(c.queries[q])
        if key in seen:                                       # (the table sequence repeats queries)
            continue
        seen.add(key)
        plan, got = c.plan(q), oracle_numbers(name, q)
        assert len(plan) == len(got) == len(c.declared[q])
        for r, (p, g, d) in enumerate(zip(plan, got, c.declared[q])):
            for f in PLAN_FIELDS:
                assert getattr(p, f) == g[f], f"{name} query {q} row {r}: {f} planned {getattr(p, f)}, the oracle says {g[f]}"
            for f, v in (d or {}).items():
                assert g[f] == v, f"{name} query {q} row {r}: built for {f} = {v}, the oracle says {g[f]}"


@pytest.mark.parametrize("name", S.all_names())
def test_rows_that_may_leave_are_an_interval(name, oracle_numbers):
    c = S.case(name)
    for q in range(len(c.queries)):
        cols = [g["columns"] for g in oracle_numbers(name, q)]
        lo, hi = c.expected_overflow(q)
        assert (lo, hi) == S.overflow_interval(cols)
        assert lo == sum(x >= S.QJ_LIMIT + S.QJ_T for x in cols) and hi - lo == sum(S.QJ_LIMIT < x < S.QJ_LIMIT + S.QJ_T for x in cols)
        assert c.expected_may_overflow(q) == sum(g["lookups"] > S.QJ_LIMIT for g in oracle_numbers(name, q))


def test_the_limit_sweep_states_what_the_issue_asks():
    want = {S.QJ_LIMIT - 1: (0, 0), S.QJ_LIMIT: (0, 0), S.QJ_LIMIT + 1: (0, 1), S.MUST_LEAVE - 1: (0, 1), S.MUST_LEAVE: (1, 1),
            S.QJ_HT - 1: (1, 1), S.QJ_HT: (1, 1), S.QJ_HT + 1: (1, 1)}
    assert set(S.A_COLUMNS) == set(want)
    for layout in ("single", "spread"):
        for C_, iv in want.items():
            c = S.case(f"A-{layout}-{C_}")
            assert c.expected_overflow(0) == iv and c.expected_may_overflow(0) == 1
            p = c.plan(0)[0]
            assert p.columns == C_ and 0 < p.cells < p.columns          # keys are not cells
            assert p.records == (12 if layout == "single" else 1800)
    assert S.case("B-few").expected_may_overflow(0) == 1 and S.case("B-few").expected_overflow(0) == (0, 0)
    assert S.case("B-few").plan(0)[0].columns <= S.QJ_LIMIT // 2 and S.case("B-few").plan(0)[0].lookups > S.QJ_LIMIT
    assert S.case("B-limit").plan(0)[0].lookups == S.QJ_LIMIT and S.case("B-limit").expected_may_overflow(0) == 0
    assert S.case("B-limit+1").plan(0)[0].lookups == S.QJ_LIMIT + 1 and S.case("B-limit+1").expected_may_overflow(0) == 1


def test_the_chunk_cases_put_their_records_where_they_say():
    for R in S.C_RECORDS:
        assert S.case(f"C-records-{R}").plan(0)[0].records == R
    sz = S.case("C-edges").plan(0)[0].sizes
    for at in (0, S.QJ_T - 1, S.QJ_T, 2 * S.QJ_T - 1, 2 * S.QJ_T):
        assert sz[at] == 0                                    # zero-size records first and last in a chunk
    assert all((sz[c * S.QJ_T:(c + 1) * S.QJ_T] >= 2).sum() >= 20 for c in range(3))
    sz = S.case("C-dead_chunk").plan(0)[0].sizes
    assert (sz[:S.QJ_T] >= 2).any() and not sz[S.QJ_T:2 * S.QJ_T].any() and (sz[2 * S.QJ_T:] >= 2).any()
    p = S.case("C-all_dead").plan(0)[0]
    assert p.records > 3 * S.QJ_T and p.groups == p.cells == 0
    for t in (255, 256, 257):
        assert S.case(f"C-total_{t}").plan(0)[0].chunk_lookups[:2] == [t, t + S.QJ_T]
    sz = S.case("C-one_long").plan(0)[0].sizes
    live = sz[sz > 0]
    at = int(np.argmax(live))
    assert live[at] == 300 > S.QJ_T and 0 < at < len(live) - 1 and set(np.delete(live, at).tolist()) == {2}
    for chunk in (1, 2):
        p = S.case(f"D-leaves-in-chunk-{chunk}").plan(0)[0]
        keys = 24 + np.cumsum(np.where(p.sizes > 3, p.sizes - 1, 0))      # (the early words share 24 columns; every later lookup is a new one)
        assert keys[chunk * S.QJ_T - 1] == 24 and keys[-1] == p.columns >= S.MUST_LEAVE
        crossing = int(np.searchsorted(keys, S.QJ_LIMIT))
        assert chunk * S.QJ_T + 64 < crossing < (chunk + 1) * S.QJ_T - 64     # in the middle of the chunk


def test_the_many_rows_cases_differ_from_row_to_row():
    for rows in S.E_ROWS:
        c = S.case(f"E-{rows}-rows")
        plan = c.plan(0)
        assert len(plan) == rows and c.expected_overflow(0) == (rows, rows)
        assert all(p.columns > S.MUST_LEAVE and 0 < p.cells < p.columns for p in plan)
        assert len({p.cells for p in plan}) == rows and len({(p.lookups, p.cells) for p in plan}) == rows
    assert {r > S.QH_WG for r in S.E_ROWS} == {False, True} and S.QH_WG in S.E_ROWS and 2 * S.QH_WG + 1 in S.E_ROWS


def test_the_table_sequence_follows_the_bookkeeping():
    steps = S.table_steps()
    assert S.model_tables(steps, False) == [s[2] for s in steps]
    assert S.model_tables(steps, True) == [s[3] for s in steps]
    c = S.case("F-tables")
    assert sum(len(s[1]) for s in steps) == len(c.queries)
    for q in range(len(c.queries)):                           # every planted row of the sequence must leave: the model counts on it
        planted = sum(isinstance(r, S.QRow) for r in c.queries[q])
        assert c.expected_overflow(q) == (planted, planted)
    kinds = [(s[0], max(len(x) for x in s[1])) for s in steps]
    assert ("batch", 21) in kinds and ("single", 21) in kinds and ("single", 20) in kinds and ("single", 19) in kinds
    assert any(s[2][2] == 0 for s in steps) and any(s[2][1] == S.QH_WG for s in steps)


@pytest.mark.parametrize("name,n", [(f"A-single-{S.MUST_LEAVE}", 1), (f"A-spread-{S.QJ_HT}", 2), ("D-leaves-in-chunk-2", 1), ("E-17-rows", 17),
                                    ("F-tables", 21), ("C-edges", 1)])
def test_the_probe_row_has_a_cell_in_every_planted_column(name, n):
    from oracle import binding as ob
    c = S.case(name)
    rows = c.probe(n)
    assert len(rows) == n
    res, off, gen, G = c.union(rows)
    ora = ob.Oracle(res, off, gen, S.K)
    got = S.from_oracle(ora.dictionary(), ora.scores(G), c.N, n)
    ora.close()
    plan = [S.plan_row(c, rows, r) for r in range(n)]
    for p, g in zip(plan, got):
        for f in PLAN_FIELDS:
            assert getattr(p, f) == g[f], (name, f)
    assert got[0]["cells"] == got[0]["columns"] == c.n_col - 2 and all(g["cells"] == 0 for g in got[1:])


def test_query_join_info_matches_the_header(tmp_path):
    from pandelos_amd import _lib
    fields = [n for n, _ in _lib.PdlQueryJoinInfo._fields_]
    assert fields == ["rows", "may_overflow_rows", "overflow_rows", "hbm_launches", "hbm_workgroups", "hbm_clears"]
    src, exe = tmp_path / "size.c", tmp_path / "size"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pandelos_amd.h"\nint main(void) { printf("%zu", sizeof(pdl_query_join_info));\n'
                   + "".join(f'printf(" %zu", offsetof(pdl_query_join_info, {n}));\n' for n in fields) + "return 0; }\n")
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    size, *offs = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert C.sizeof(_lib.PdlQueryJoinInfo) == size
    assert [getattr(_lib.PdlQueryJoinInfo, n).offset for n in fields] == offs
    assert "pdl_get_query_join_info" in _lib.EXPORTS


@pytest.mark.parametrize("lib", ["libpandelos_amd.so", "libnative.so"])
def test_libraries_export_the_getter(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "pandelos_amd" / "lib" / lib)], check=True, capture_output=True, text=True).stdout
    assert any(line.split()[-1] == "pdl_get_query_join_info" for line in out.splitlines() if line.strip())


# ---- the cases outside the word construction ---------------------------------------------------------------------------------------
def _raw_numbers(c, rows):
    """from the oracle's dictionary of the union: (lookups of EVERY query row, {row: distinct columns} for `rows`, the block)"""
    from oracle import binding as ob
    res, off, gen, G = c.union()
    ora = ob.Oracle(res, off, gen, S.K)
    r, gid, start, size = H.rank_groups(ora.dictionary())
    block = ora.scores(G)
    kseq = ora.kseq_lengths().copy()
    ora.close()
    seq = r["seq"].astype(np.int64)
    sz = size[gid]
    lookups = np.bincount(seq, weights=np.where(sz >= 2, sz, 0), minlength=c.N + len(c.query_genes)).astype(np.int64)[c.N:]
    cols = {}
    for g in rows:
        mine = np.flatnonzero((seq == c.N + g) & (sz >= 2))
        members = set()
        for i in mine.tolist():
            members.update(seq[start[gid[i]]:start[gid[i]] + size[gid[i]]].tolist())
        members.discard(c.N + g)
        cols[g] = members
    return lookups, cols, block, kseq


@pytest.mark.parametrize("name", S.names_g())
def test_the_fold_cases_fold_what_they_say(name):
    c = S.raw_case(name)
    variant, wide = name.split("-")[1], name.endswith("wide")
    W = S.FOLD_WIDE if wide else S.FOLD_BELOW
    assert S.FOLD_WIDE >= S.MUST_LEAVE and S.FOLD_BELOW + 2 <= S.QJ_LIMIT
    n = len(c.query_genes)
    rows = [0, 1, 2] if n == 3 else [0, n // 2, n - 1]
    lookups, cols, block, _ = _raw_numbers(c, rows)
    assert int((lookups > S.QJ_LIMIT).sum()) == c.may_overflow
    for g in rows:
        assert len(cols[g]) == c.columns[g], (name, g, len(cols[g]))
    assert c.expected_overflow() == ((sum(x >= W for x in c.columns), ) * 2 if wide else (0, 0))
    N = c.N
    if variant == "qextra":          # the one record of ZACDE, the union's last, has the W holders of YYYYY and the query's holder as columns
        assert lookups[0] == W + 2 and cols[0] == set(range(W)) | {N + 1} and cols[1] == set(range(W)) | {N}
    elif variant == "bskip":         # T left the group of YYYYW: the query's YYYYW row has the W holders, and T belongs to the query's YYYYY
        T = c.note["T"]
        assert cols[0] == {T} and T not in cols[1] and len(cols[1]) == W and lookups[1] == W + 1
    else:                            # T joined the query's group of YYYYW
        T = c.note["T"]
        for g in rows:
            assert T in cols[g] and cols[g] - {T} == set(range(N, N + n)) - {N + g}


@pytest.mark.parametrize("name", S.names_h())
def test_the_large_sums_are_what_they_say(name):
    c = S.raw_case(name)
    lookups, cols, block, kseq = _raw_numbers(c, [0, 1])
    assert len(cols[0]) == c.columns[0] and len(cols[1]) == c.columns[1] and {0, 1, 2} <= cols[0]
    assert int((lookups > S.QJ_LIMIT).sum()) == c.may_overflow and c.expected_overflow() == ((1, 1) if name.endswith("hbm") else (0, 0))
    assert kseq.max() < S.GENE_KMERS_GUARD and kseq[c.N] > S.GENE_KMERS_GUARD - 2100

    def counts(g):
        w, n = S.row_windows(g)
        return dict(zip(w.tolist(), n.tolist()))
    mine = counts(c.query_genes[0])
    for col in (0, 1, 2):
        other = counts(c.base_genes[col])
        shared = set(mine) & set(other)
        inter, pc, tc = (sum(min(mine[x], other[x]) for x in shared), sum(mine[x] for x in shared), sum(other[x] for x in shared))
        assert pc >= S.L_SUM > (1 << 20) - 2100 and pc < 1 << 20          # the row's sum fills 20 bits of its 21-bit field
        if col == 0:
            assert inter == tc == pc
        else:
            assert inter == tc < pc and inter > 1 << 19
        at = np.flatnonzero((np.asarray(block["row"]) == c.N) & (np.asarray(block["column"]) == col))
        assert len(at) == 1
        assert block["percs"][at[0]] == np.float32(pc) / np.float32(int(kseq[c.N]))
        assert block["tr_percs"][at[0]] == np.float32(tc) / np.float32(int(kseq[col]))
        assert block["scores"][at[0]] == np.float32(inter) / np.float32(int(kseq[c.N]) + int(kseq[col]) - inter)


def test_the_walk_s_search_is_held_by_the_zero_size_records():
    """q_walk_row's search, restated in numpy (query_join_sets.walk_chunk), over the chunks of C-edges and C-dead_chunk: with `<=`
    every lookup lands on a live record, at a member inside its group, each (record, member) once; with `<` it does not — the first
    lookup of a record behind a live one becomes member `size` of the record in front, one past its group."""
    for name in ("C-edges", "C-dead_chunk", "C-one_long", "C-total_256"):
        sizes = S.case(name).plan(0)[0].sizes
        wrong = 0
        for c0 in range(0, len(sizes), S.QJ_T):
            sz = sizes[c0:c0 + S.QJ_T]
            got = S.walk_chunk(sz)
            want = [(i, m) for i, n in enumerate(sz.tolist()) for m in range(n)]
            assert got == want, (name, c0)
            strict = S.walk_chunk(sz, strict=True)
            wrong += sum(m >= sz[i] or sz[i] == 0 for i, m in strict)
            assert strict != want or not want
        assert wrong >= (sizes > 0).sum() - len(range(0, len(sizes), S.QJ_T)), name


def test_rows_carried_over_the_limit_by_genes_of_their_own_query():
    c = S.raw_case("I-query-columns")
    n = len(c.query_genes)
    lookups, cols, block, _ = _raw_numbers(c, [0, n // 2, n - 1])
    assert int((lookups > S.QJ_LIMIT).sum()) == c.may_overflow == n and c.expected_overflow() == (n, n)
    for g, members in cols.items():
        assert len(members) == c.columns[g] == S.MUST_LEAVE
        assert sum(m < c.N for m in members) == S.I_BASE <= S.QJ_LIMIT and members >= set(range(c.N, c.N + n)) - {c.N + g}


@pytest.mark.parametrize("name", S.raw_names())
def test_a_raw_case_s_queries_bring_no_letter_the_base_lacks(name):
    c = S.raw_case(name)
    have = set(np.unique(c.base[0]).tolist())
    assert set(np.unique(c.query()[0]).tolist()) <= have
    assert set(S.JE.filler(26001, 15).tolist()) | set(S.JE.filler(26002, 15).tolist()) <= have       # the small queries beside it in a batch
