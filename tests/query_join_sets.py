"""Query genomes with PLANTED rows for the query's join (pandelos_amd/csrc/pdl_query.h: q_walk_row, q_row_lds, q_row_hbm, k_q_join,
k_q_join_hbm; pdl_query_batch.h: k_qb_join, k_qb_join_hbm): rows whose records, groups, lookups per chunk of 256 records and
distinct columns are decided before anything runs, so that a row can be put ON the LDS table's limit, on a chunk's edge, or into a
sequence of calls that grows and relays the tables in HBM.  Pure numpy, no device.

The construction is that of tests/join_edge_sets.py (its words, fillers, column separator and trailing genes, imported): the
COLUMNS are base genes, the planted rows are the genes of the QUERY genome.

  words     five payload letters, spread evenly over the 13^5 there are: lexicographic order = rank order = order of the word's index
  a column  base gene c: the words it holds (as often as its count says), a W behind each, then its filler
  a row     query gene r: its words in index order (twice where its own count is 2), each followed by the row's SEPARATOR — a byte no
            other gene of the union holds except the base's alphabet gene — and a tail of separators.  The four separators of
            join_edge_sets (Q R S T) come first, then B J O U X and the bytes '!' .. '@': 41 rows at the most.  Every window that
            spans a join holds the separator, so it is the row's alone: a record of its own with a group of one — a ZERO-SIZE record
            of the walk (q_walk_row: sz < 2).  A planted row therefore always has such records between its words, about five to a word,
            and where a word stands in the row's rank order is known from the row's own string (`row_windows`).
  a word's  group in the union: the base columns that hold it and the rows OF THE SAME QUERY that hold it.  A word nobody else holds is
            one more zero-size record.
  dead row  a query gene that is a filler of its own: five records, all of size one — no cell, but a row of the join
  base      columns, padding, the alphabet gene (V s V s ... over every separator: the query's letters are the base's, and its windows
            hold two V or more, which no other gene's do), then the two trailing genes of join_edge_sets that hold YYYYY: the largest
            k-mer of every union, in a group of two, so neither the base's fold nor the union's moves a record (pdl_query.h, Q1).

A row's PLAN follows from the incidence and the row's own string alone (`plan_row`): its records, the records with a group of two or
more, the lookups as the kernels count them (a group's size, the row itself included: k_q_match's row_lookups, what k_q_row_off
holds against QJ_LIMIT), the lookups of every chunk of QJ_T records, the distinct columns (the row itself NOT counted: its cell is
never made, q_walk_row), and the cells the row emits (library.cpp:493-517 in float32).  tests/test_query_join_sets_cpu.py recomputes
every number from the CPU oracle's dictionary and block of the union and holds each case's own declaration against both.

The constants restate the kernels'; tests/test_query_join_sets_cpu.py reads them out of the source, so a limit that moves fails
there with its name."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from tests import helpers as H
from tests import join_edge_sets as JE

K = JE.K
QJ_T = 256                                  # pdl_query.h:336  records per chunk of the walk = threads of a workgroup
QJ_HT_BITS = 12                             # pdl_query.h:337
QJ_HT = 1 << QJ_HT_BITS                     # pdl_query.h:337  slots of the LDS table
QJ_LIMIT = QJ_HT - 2 * QJ_T                 # pdl_query.h:338  keys a row may claim before it goes to the HBM tables: 3584
QH_WG = 16                                  # pdl_query.h:340  workgroups (tables) of the HBM kernel at the most
GENE_KMERS_GUARD = 1 << 20                  # pdl_query.h (pdl_run_query_device), pdl_query_batch.h (pdl_query_batch_plan): genes below 2^20 k-mers
FIELD_BITS = 21                             # pdl_query.h:412  the packed accumulator: three sums of 21 bits
SOURCE_CONSTANTS = {"QJ_T": QJ_T, "QJ_HT_BITS": QJ_HT_BITS, "QH_WG": QH_WG}
MUST_LEAVE = QJ_LIMIT + QJ_T                # the limit is tested before the atomicCAS: up to QJ_T - 1 further keys can land

SEPARATORS = JE.ROW_SEPARATORS + b"BJOUX" + bytes(range(0x21, 0x41))
assert len(set(SEPARATORS)) == len(SEPARATORS) and not set(SEPARATORS) & set(JE.PAYLOAD.tolist()) \
    and not set(SEPARATORS) & {JE.COLUMN_SEPARATOR, JE.FILLER_MARK, JE.TOP_LETTER} and max(SEPARATORS) < JE.TOP_LETTER


AUX_SEP = len(SEPARATORS) - 2               # the separator of small_queries' row: in every base's alphabet
PROBE_SEP = len(SEPARATORS) - 1             # ... and that of the probe row


def overflow_interval(columns) -> tuple:
    """rows that leave the LDS table, as (fewest, most): a row of C distinct columns stays with C <= QJ_LIMIT, leaves with
    C >= QJ_LIMIT + QJ_T, and may do either in between"""
    c = np.asarray(columns, np.int64)
    return int((c >= MUST_LEAVE).sum()), int((c > QJ_LIMIT).sum())


# ---- incidence -----------------------------------------------------------------------------------------------------------------
@dataclass
class QRow:
    """A planted row of a query: `words` = [(word index, own count)], `sep` = index of its separator, `tail` separators behind"""
    words: list
    sep: int
    tail: int = 12


@dataclass
class Dead:
    """A query gene that shares nothing: a filler under an id of its own"""
    ident: int


def word_letters(nw: int) -> list:
    """the letters of nw words, as join_edge_sets.planted_rows spreads them"""
    stride = JE.WORDS // nw
    assert stride >= 1
    stride -= stride > 1 and stride % 13 == 0
    return [JE.word(int(i * stride)) for i in range(nw)]


def row_string(letters, row) -> np.ndarray:
    if isinstance(row, Dead):
        return JE.filler(row.ident, 15)
    s = np.array([SEPARATORS[row.sep]], np.uint8)
    parts = []
    for w, own in sorted(row.words):
        parts += [letters[w], s] * own
    out = np.concatenate(parts + [np.repeat(s, max(row.tail, 0))])
    return out[:row.tail] if row.tail < 0 else out        # (tail -1: not even the last word's separator)


def pack(windows: np.ndarray) -> np.ndarray:
    """k bytes -> one integer whose order is the k-mers' rank order (the rank table ascends with the byte value)"""
    v = np.zeros(len(windows), np.int64)
    for j in range(K):
        v = v * 256 + windows[:, j].astype(np.int64)
    return v


def row_windows(s: np.ndarray):
    """-> (the row's distinct k-mers in rank order, packed; the count of each): its records"""
    if len(s) < K:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.unique(pack(np.lib.stride_tricks.sliding_window_view(s, K)), return_counts=True)


def word_positions(letters, row: QRow) -> dict:
    """{word index: position of the word's record among the row's records}"""
    wins, _ = row_windows(row_string(letters, row))
    return {w: int(np.searchsorted(wins, pack(letters[w][None, :])[0])) for w, _ in row.words}


@dataclass
class RowPlan:
    records: int                    # records of the row (distinct k-mers of the gene)
    groups: int                     # ... whose group has two members or more
    lookups: int                    # sum of those groups' sizes, the row itself included: row_lookups of k_q_match
    chunk_lookups: list             # ... of every chunk of QJ_T records
    columns: int                    # distinct columns, the row itself not counted
    cells: int                      # cells the row emits
    sizes: np.ndarray = None        # per record, in rank order: the group's size (0 below two)


@dataclass
class Case:
    """k = 5, a base and one or more queries.  holders[w] = (base columns of word w, ascending; their counts of it)."""
    name: str
    nw: int
    n_col: int
    holders: dict
    queries: list                   # [[QRow | Dead]]
    padding: int = 0
    as_batch: bool = False          # the queries are ONE batch (else: one query, or a sequence of calls)
    declared: list = None           # per query, per row: {plan field: the number the case was built for} (None: nothing declared)
    note: dict = field(default_factory=dict)
    extra_seps: tuple = ()          # separators the base's alphabet gene holds besides those of the case's own rows

    @functools.cached_property
    def letters(self): return word_letters(self.nw)

    @functools.cached_property
    def seps(self): return sorted({r.sep for q in self.queries for r in q if isinstance(r, QRow)} | {AUX_SEP, PROBE_SEP} | set(self.extra_seps))

    @functools.cached_property
    def base_genes(self) -> list:
        held = [[] for _ in range(self.n_col)]
        for w in sorted(self.holders):
            cols, ccnt = self.holders[w]
            assert len(cols) == len(ccnt) and (len(cols) == 0 or (np.all(np.diff(cols) > 0) and cols[-1] < self.n_col))
            for c, cc in zip(np.asarray(cols).tolist(), np.asarray(ccnt).tolist()):
                held[c] += [w] * cc
        sep = np.array([JE.COLUMN_SEPARATOR], np.uint8)
        genes = []
        for c in range(self.n_col):
            if not held[c]:
                genes.append(JE.filler(c, 15)); continue
            parts = []
            for w in held[c]:
                parts += [self.letters[w], sep]
            genes.append(np.concatenate(parts + [JE.filler(c, 11 if len(held[c]) == 1 else 6)]))
        n = self.n_col
        genes += [JE.filler(n + i, 15) for i in range(self.padding)]
        n += self.padding
        alpha = np.array([x for s in self.seps for x in (JE.FILLER_MARK, SEPARATORS[s])] + [JE.FILLER_MARK], np.uint8)
        genes.append(np.resize(alpha, max(len(alpha), 2 * K - 1)) if len(alpha) > 1 else JE.filler(n, 15))
        for i in range(2):
            genes.append(np.r_[np.full(K + 1, JE.TOP_LETTER, np.uint8), JE.filler(n + 1 + i, 15)])
        return genes

    @property
    def N(self): return self.n_col + self.padding + 3

    @functools.cached_property
    def base(self):
        """(residues, offsets, genome_of): three genomes"""
        genes = self.base_genes
        genome_of = np.minimum(np.arange(len(genes)) * 3 // max(len(genes), 3), 2)
        gs = H.as_gene_set(genes, genome_of, np.full(len(genes), -1))
        return gs.residues, gs.offsets, gs.genome_of

    def rows_of(self, q) -> list:
        """a query by its index, or the rows themselves"""
        return self.queries[q] if isinstance(q, int) else list(q)

    def query_genes(self, q) -> list:
        return [row_string(self.letters, r) for r in self.rows_of(q)]

    def probe(self, n: int) -> tuple:
        """The PROBE query of n genes: one row that holds the probe word (the last but one of the table: every planted column holds it
        once) twice and no tail — 8 k-mers, perc 2 / 8: a cell in EVERY planted column — and dead genes.  Run behind a case's query
        with the same gene count, it finds the tables laid out for its columns; a column an earlier row touched without emitting a
        cell, and did not reset, is missing from its block."""
        return (QRow([(self.nw - 2, 2)], PROBE_SEP, 0),) + tuple(Dead(22000 + j) for j in range(n - 1))

    def query(self, q):
        """(residues, offsets) of query q"""
        genes = self.query_genes(q)
        off = np.zeros(len(genes) + 1, np.uint64)
        np.cumsum([len(g) for g in genes], out=off[1:])
        return np.concatenate(genes).astype(np.uint8), off

    def union(self, q):
        """(residues, offsets, genome_of, G) of the base with query q as genome G"""
        rb, ob_, gb = self.base
        rq, oq = self.query(q)
        return (np.concatenate([rb, rq]).astype(np.uint8), np.concatenate([ob_, ob_[-1] + oq[1:]]).astype(np.uint64),
                np.concatenate([gb, np.full(len(oq) - 1, 3, np.uint32)]).astype(np.uint32), 3)

    @functools.lru_cache(maxsize=None)
    def plan(self, q) -> list:
        return [plan_row(self, q, r) for r in range(len(self.rows_of(q)))]

    def expected_overflow(self, q: int) -> tuple:
        return overflow_interval([p.columns for p in self.plan(q)])

    def expected_may_overflow(self, q: int) -> int:
        return sum(p.lookups > QJ_LIMIT for p in self.plan(q))

    def __hash__(self): return hash(self.name)
    def __eq__(self, other): return self is other


def plan_row(case: Case, q: int, r: int) -> RowPlan:
    """The plan of row r of query q, from the incidence (case.holders, the query's rows) and the row's own string."""
    rows = case.rows_of(q)
    N, n = case.N, len(rows)
    me = rows[r]
    s = row_string(case.letters, me)
    wins, cnt = row_windows(s)
    sizes = np.zeros(len(wins), np.int64)
    if isinstance(me, Dead):
        return RowPlan(len(wins), 0, 0, [0] * -(-len(wins) // QJ_T), 0, 0, sizes)
    assert sum(isinstance(x, QRow) and x.sep == me.sep for x in rows) == 1, "a separator belongs to one row of a query"
    kseq_b = np.array([len(g) - K + 1 for g in case.base_genes], np.int64)
    kseq_q = np.array([max(len(g) - K + 1, 0) for g in case.query_genes(q)], np.int64)
    kseq = np.r_[kseq_b, kseq_q]
    inter, pc, tc = (np.zeros(N + n, np.int64) for _ in range(3))
    for w, own in me.words:
        cols, ccnt = case.holders.get(w, (np.zeros(0, np.int64), np.zeros(0, np.int64)))
        others = [(N + i, o) for i, x in enumerate(rows) if isinstance(x, QRow) and i != r for ww, o in x.words if ww == w]
        size = len(cols) + len(others) + 1
        at = int(np.searchsorted(wins, pack(case.letters[w][None, :])[0]))
        assert cnt[at] == own
        if size < 2:
            continue
        sizes[at] = size
        col = np.r_[np.asarray(cols, np.int64), np.array([g for g, _ in others], np.int64)]
        cc = np.r_[np.asarray(ccnt, np.int64), np.array([o for _, o in others], np.int64)]
        inter[col] += np.minimum(cc, own); pc[col] += own; tc[col] += cc
    thr = np.float32(1.0) / np.float32(2.0 * K)
    touched = np.flatnonzero(pc > 0)
    valid = ((pc[touched].astype(np.float32) / np.float32(kseq[N + r]) >= thr)
             | (tc[touched].astype(np.float32) / kseq[touched].astype(np.float32) >= thr))
    return RowPlan(len(wins), int((sizes >= 2).sum()), int(sizes.sum()), [int(sizes[i:i + QJ_T].sum()) for i in range(0, len(wins), QJ_T)],
                   len(touched), int(valid.sum()), sizes)


def from_oracle(dictionary, block, N: int, n: int) -> list:
    """What plan_row states, taken instead from the CPU oracle's dictionary of the union (records {rank, seq, count}) and its block of
    genome G: [per query gene: {records, groups, lookups, chunk_lookups, columns, cells}]"""
    r, gid, start, size = H.rank_groups(dictionary)
    seq = r["seq"].astype(np.int64)
    cells = np.bincount(np.asarray(block["row"], np.int64) - N, minlength=n) if len(block["row"]) else np.zeros(n, np.int64)
    out = []
    for g in range(N, N + n):
        mine = np.flatnonzero(seq == g)                   # (rank order: the groups ascend by rank)
        sz = size[gid[mine]]
        sz = np.where(sz >= 2, sz, 0)
        cols = set()
        for i in mine[sz >= 2].tolist():
            lo = int(start[gid[i]])
            cols.update(seq[lo:lo + int(size[gid[i]])].tolist())
        cols.discard(g)
        out.append({"records": len(mine), "groups": int((sz >= 2).sum()), "lookups": int(sz.sum()),
                    "chunk_lookups": [int(sz[i:i + QJ_T].sum()) for i in range(0, len(mine), QJ_T)], "columns": len(cols),
                    "cells": int(cells[g - N])})
    return out


# ---- small parts ---------------------------------------------------------------------------------------------------------------
def ones(n): return np.ones(n, np.int64)


def holders_of(row: JE.Row, first_word: int = 0) -> dict:
    """the ranges of a join_edge_sets Row as words first_word, first_word + 1, ...: {word: (columns, counts)}"""
    return {first_word + i: (row.cols[i], row.ccnt[i]) for i in range(row.nr)}


def row_of(row: JE.Row, sep: int, first_word: int = 0, tail: int = 12) -> QRow:
    return QRow([(first_word + i, int(row.own[i])) for i in range(row.nr)], sep, tail)


def small_queries(case_nw: int):
    """the two unrelated queries a single-query case stands between in a batch: a row on the auxiliary word (the LAST word of every
    case's table, held by the last two base columns) beside a dead gene; a dead gene alone"""
    return [[QRow([(case_nw - 1, 1)], AUX_SEP), Dead(20001)], [Dead(20002)]]


def with_aux(holders: dict, nw: int, n_col: int) -> dict:
    """... and that word's holders; the probe word (Case.probe), held once by every column in front of those two"""
    holders = dict(holders)
    assert nw - 1 not in holders and nw - 2 not in holders
    holders[nw - 1] = (np.array([n_col - 2, n_col - 1]), np.array([2, 2]))
    holders[nw - 2] = (np.arange(n_col - 2), ones(n_col - 2))
    return holders


# ---- the cases -------------------------------------------------------------------------------------------------------------------
A_COLUMNS = (QJ_LIMIT - 1, QJ_LIMIT, QJ_LIMIT + 1, MUST_LEAVE - 1, MUST_LEAVE, QJ_HT - 1, QJ_HT, QJ_HT + 1)
C_RECORDS = (1, 255, 256, 257, 511, 512, 513)
E_ROWS = (15, 16, 17, 33)
WIDTHS = (64, 65, 256, 257, 512, 513)


def _single(name, nw, n_col, holders, rows, declared, **kw) -> Case:
    """one query of `rows`; the last word and the last two columns are the auxiliary ones of small_queries, the last word but one is
    the probe's"""
    return Case(name, nw, n_col + 2, with_aux(holders, nw, n_col + 2), [rows], declared=[declared], **kw)


def case_a(layout: str, C: int) -> Case:
    """Columns at the table limit: ONE row of exactly C distinct columns.
    "single": one record holds them all; a second one holds the first 40 again, which therefore have two sightings and a cell —
              the others are touched and emit nothing: keys are not cells.
    "spread": 300 records deal 3 C / 2 lookups round the C columns: half of the columns have two sightings and a cell."""
    if layout == "single":
        row = JE.Row([np.arange(C), np.arange(40)])
        cells = 40
    else:
        row = JE.cyclic(JE.even_lens(300, C + C // 2), C)
        cells = C // 2
    nw = row.nr + 2
    return _single(f"A-{layout}-{C}", nw, C, holders_of(row), [row_of(row, 0)],
                   [{"columns": C, "groups": row.nr, "lookups": row.lookups + row.nr, "cells": cells}])


def case_b(kind: str) -> Case:
    """Many lookups, few columns.  "few": 300 records of 13 columns dealt round QJ_LIMIT / 2 columns — 4200 lookups: the prefilter
    counts the row, the table holds it, the host reads the overflow word and launches nothing.  "limit": exactly QJ_LIMIT lookups as
    k_q_row_off counts them (the row itself once per record), every column another one: not counted.  "limit+1": one lookup more."""
    if kind == "few":
        row = JE.cyclic([13] * 300, QJ_LIMIT // 2)
        C = QJ_LIMIT // 2
    else:
        nr = 64
        row_lookups = QJ_LIMIT + (kind == "limit+1")
        lens = JE.even_lens(nr, row_lookups - nr)
        row = JE.Row([np.arange(a, a + n) for a, n in zip(np.r_[0, np.cumsum(lens)[:-1]].tolist(), lens.tolist())])
        C = row_lookups - nr
    return _single(f"B-{kind}", row.nr + 2, C, holders_of(row), [row_of(row, 1)], [{"columns": C, "lookups": row.lookups + row.nr}])


def _row_with_records(letters, records: int, sep: int):
    """a row of exactly `records` records: its first n words and a tail, searched over n and the tail's length"""
    for n in range(max(records // 6 - 2, 1), records // 6 + 3):
        for tail in range(-1, 5):                         # (6 n - 4 + min(tail, 4) records: the tail's windows are new ones up to QQQQQ)
            row = QRow([(w, 1) for w in range(n)], sep, tail)
            if len(row_windows(row_string(letters, row))[0]) == records:
                return row
    raise AssertionError(records)


def case_c_records(R: int) -> Case:
    """A row of exactly R records; every word is held by two of 24 columns dealt round, and with its own count the row has a cell
    in each.  R = 1: the gene is one word."""
    nw = 100
    letters = word_letters(nw)
    row = QRow([(0, 1)], 2, -1) if R == 1 else _row_with_records(letters, R, 2)      # (R = 1: a gene of k letters, no separator at all)
    m = len(row.words)
    inc = JE.cyclic([2] * m, 24)
    return _single(f"C-records-{R}", nw, 24, holders_of(inc), [row], [{"records": R, "groups": m, "lookups": 3 * m, "columns": min(24, 2 * m)}])


def _long_row(nw: int, words: int, sep: int):
    letters = word_letters(nw)
    row = QRow([(w, 1) for w in range(words)], sep, 12)
    return letters, row, word_positions(letters, row)


def case_c_pattern(kind: str) -> Case:
    """A row of 130 words — 780 records and more, four chunks, the words among the first 650 or so — whose words are LIVE (held by base columns) or not by where their
    record stands in the row's rank order:
      "edges"       the first and the last record of chunks 0 and 1 are zero-size (a word left alone where a word stands there),
                    their neighbours live
      "dead_chunk"  chunk 1 holds zero-size records only; chunks 0 and 2 are live
      "all_dead"    no word is held by anybody: records, no group, no cell
      "total_255" / "total_256" / "total_257"   chunk 0's lookups add up to just that, chunk 1's to 256 more
      "one_long"    one record of 300 lookups (299 columns without a cell) between records of two (a column with a cell each)"""
    nw = 140
    letters, row, pos = _long_row(nw, 130, 3)
    n_chunks = -(-len(row_windows(row_string(letters, row))[0]) // QJ_T)
    chunk = {w: p // QJ_T for w, p in pos.items()}
    by_pos = sorted(pos, key=pos.get)
    holders, n_col, declared = {}, 440, {}
    if kind == "edges":
        dead = {w for w, p in pos.items() if p % QJ_T in (0, QJ_T - 1)}
        for i, w in enumerate(by_pos):
            if w not in dead:
                holders[w] = (np.array([(2 * i) % 24, (2 * i) % 24 + 1]), ones(2))
        declared = {"groups": 130 - len(dead)}
    elif kind == "dead_chunk":
        for i, w in enumerate(by_pos):
            if chunk[w] != 1:
                holders[w] = (np.array([(2 * i) % 24, (2 * i) % 24 + 1]), ones(2))
        declared = {"groups": sum(c != 1 for c in chunk.values())}
    elif kind == "all_dead":
        declared = {"groups": 0, "lookups": 0, "columns": 0, "cells": 0}
    elif kind.startswith("total_"):
        want = int(kind[6:])
        for c, total in ((0, want), (1, want + QJ_T)):
            ws = [w for w in by_pos if chunk[w] == c]
            lens = JE.even_lens(len(ws), total - len(ws))             # (a group's size counts the row itself)
            at = 0
            for w, n in zip(ws, lens.tolist()):
                holders[w] = (np.arange(at, at + n) % n_col, ones(n)); at += n
                holders[w] = (np.sort(holders[w][0]), ones(n))
        declared = {"chunk_lookups": [want, want + QJ_T] + [0] * (n_chunks - 2)}
    elif kind == "one_long":
        mid = by_pos[len(by_pos) // 2]
        for i, w in enumerate(by_pos):
            holders[w] = (np.arange(299), ones(299)) if w == mid else (np.array([300 + i]), 2 * ones(1))      # (a count of 2: 14 k-mers, a cell)
        declared = {"groups": 130, "lookups": 300 + 2 * 129, "columns": 299 + 129, "cells": 129}
    else:
        raise KeyError(kind)
    return _single(f"C-{kind}", nw, n_col, holders, [row], [declared], note={"positions": pos})


def case_d(chunk: int) -> Case:
    """Leaving late: the words of the chunks in front of `chunk` (1 or 2) hold two of 24 columns each; from that chunk on every word
    brings 150 new columns, so the key count passes QJ_LIMIT at the 24th word or so — in the middle of the chunk — and the row's
    LDS state is thrown away for the walk on the HBM tables."""
    nw = 160
    letters, row, pos = _long_row(nw, 150, 0)
    by_pos = sorted(pos, key=pos.get)
    holders, at = {}, 24
    for i, w in enumerate(by_pos):
        if pos[w] // QJ_T < chunk:
            holders[w] = (np.array([(2 * i) % 24, (2 * i) % 24 + 1]), ones(2))
        else:
            holders[w] = (np.arange(at, at + 150), ones(150)); at += 150
    late = sum(pos[w] // QJ_T >= chunk for w in by_pos)
    in_chunk = sum(pos[w] // QJ_T == chunk for w in by_pos)
    assert in_chunk >= 40                                 # LIMIT is passed at the 24th of them
    c = _single(f"D-leaves-in-chunk-{chunk}", nw, at, holders, [row], [{"columns": 24 + 150 * late}])
    first_chunks = sum(2 + 1 for w in by_pos if pos[w] // QJ_T < chunk)
    assert first_chunks < QJ_LIMIT // 8
    return c


# The many-rows cases, the table sequence and the widths share ONE base: 4000 columns, three wide words (0, 1, 2) of 3860 columns each,
# word j on columns [40 j, 40 j + 3860), and 41 small words (3 + i) of 20 + i columns [60 i, 60 i + 20 + i), which the wide words
# cover.  Row i of a query holds wide word i % 3, once or twice (i % 2), and small word i once.  It is 20 (26) k-mers long, so a
# column that shares the wide word alone has perc 1 / 20 (2 / 26) and, being 13 k-mers or more itself, no cell; one that shares the
# small word too has 2 / 20 (3 / 26) and a cell.  Rows i and i + 3 share their wide word, so they are columns of each other — with
# other counts, and without a cell.  The columns differ from row to row: 3860 of the base and the query's other rows on the word.
M_COLS, M_WIDE, M_SMALL = 4000, 3860, 41
M_NW = 3 + M_SMALL + 2


def m_holders() -> dict:
    h = {j: (np.arange(40 * j, 40 * j + M_WIDE), ones(M_WIDE)) for j in range(3)}
    for i in range(M_SMALL):
        h[3 + i] = (np.arange(60 * i, 60 * i + 20 + i), ones(20 + i))
    return h


def m_row(i: int) -> QRow:
    return QRow([(i % 3, 1 + i % 2), (3 + i, 1)], i)


def m_query(rows, n: int) -> list:
    """the rows `rows` of the many-rows base and dead genes up to n genes"""
    rows = list(rows)
    return [m_row(i) for i in rows] + [Dead(21000 + j) for j in range(n - len(rows))]


def m_declared(rows, n: int) -> list:
    rows = list(rows)
    return [{"columns": M_WIDE + sum(j != i and j % 3 == i % 3 for j in rows), "cells": 20 + i, "groups": 2} for i in rows] + [{"groups": 0}] * (n - len(rows))


def case_e(rows: int) -> Case:
    """15, 16, 17 and 33 rows of more than QJ_LIMIT + QJ_T columns in one query: as many workgroups as rows, or QH_WG of them that
    walk several rows each on the same tables"""
    return Case(f"E-{rows}-rows", M_NW, M_COLS + 2, with_aux(m_holders(), M_NW, M_COLS + 2), [m_query(range(rows), rows)],
                declared=[m_declared(range(rows), rows)])


# Tables across calls, on one context (q_join_hbm_tier's hbm_clean, hbm_cols, hbm_slots): (kind, queries, (hbm_launches,
# hbm_workgroups, hbm_clears) when every batch is one chunk, ... when every query is a chunk of its own).  Steps follow each other on a
# context whose tables are in no known state before the first.
def table_steps():
    q = m_query
    wide_batch = [q([0, 1], 21), q([5], 10), q([2, 3, 4], 21)]
    return [
        ("single", [q([0, 1], 20)], (1, 2, 1), (1, 2, 1)),           # tables for N + 20 columns, two slots
        ("single", [q([0, 1], 20)], (1, 2, 0), (1, 2, 0)),           # ... taken as they are
        ("single", [q(range(5), 20)], (1, 5, 1), (1, 5, 1)),         # the same columns, the slots grow 2 -> 5
        ("single", [q([6, 7], 20)], (1, 2, 0), (1, 2, 0)),           # five slots serve two rows
        ("batch", [q(range(17), 20), q([1], 20)], (1, 16, 1), (2, 16, 1)),    # 5 -> 16 slots; chunked: 17 rows, then one on the same tables
        ("single", [q([0, 1], 21)], (1, 2, 1), (1, 2, 1)),           # one column more: laid out again
        ("batch", wide_batch, (1, 6, 1), (3, 3, 1)),                 # the widest query decides N + 21; six rows on two slots: cleared.  Chunked: 2, 1, then 3 rows
        ("single", [q([8, 9], 21)], (1, 2, 0), (1, 2, 0)),           # a single query with exactly that hbm_cols behind it
        ("batch", wide_batch, (1, 6, 0), (3, 3, 0)),                 # ... and the batch once more: nothing to clear
        ("single", [q([0], 19)], (1, 1, 1), (1, 1, 1)),              # one column fewer
    ]


def model_tables(steps, chunked: bool):
    """q_join_hbm_tier's bookkeeping restated: -> [(launches, workgroups, clears)] of every step"""
    clean, cols, slots, out = False, 0, 0, []
    for kind, queries, _, _ in steps:
        n_max = max(len(x) for x in queries)
        groups = [[x] for x in queries] if (chunked or kind == "single") else [queries]
        launches = wg = clears = 0
        for grp in groups:
            n_over = sum(isinstance(r, QRow) for x in grp for r in x)         # (every planted row of these queries must leave)
            if not n_over:
                continue
            W = min(n_over, QH_WG)
            n_cols = case_f().N + (n_max if kind == "batch" else len(grp[0]))
            if not clean or cols != n_cols or slots < W:
                clean, cols, slots = True, n_cols, W
                clears += 1
            launches += 1; wg = max(wg, W)
        out.append((launches, wg, clears))
    return out


@functools.lru_cache(maxsize=None)
def case_f() -> Case:
    """every query of table_steps, in order, over the many-rows base (a step's queries are case.queries[first : first + count])"""
    queries, declared = [], []
    for kind, qs, _, _ in table_steps():
        for x in qs:
            queries.append(x)
            rows = [r.sep for r in x if isinstance(r, QRow)]
            declared.append(m_declared(rows, len(x)))
    return Case("F-tables", M_NW, M_COLS + 2, with_aux(m_holders(), M_NW, M_COLS + 2), queries, declared=declared)


def case_w(cells: int) -> Case:
    """Row widths into K-order: a row that emits exactly `cells` cells — that many columns hold both its words, 30 more only one"""
    inc = JE.Row([np.arange(cells + 30), np.arange(cells)])
    return _single(f"W-{cells}-cells", 4, cells + 30, holders_of(inc), [QRow([(0, 1), (1, 1)], 0)], [{"cells": cells, "columns": cells + 30}])


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    kind, _, arg = name.partition("-")
    if kind == "A":
        layout, _, c = arg.partition("-")
        return case_a(layout, int(c))
    if kind == "B":
        return case_b(arg)
    if kind == "C":
        return case_c_records(int(arg[8:])) if arg.startswith("records-") else case_c_pattern(arg)
    if kind == "D":
        return case_d(int(arg[-1]))
    if kind == "E":
        return case_e(int(arg.split("-")[0]))
    if kind == "F":
        return case_f()
    if kind == "W":
        return case_w(int(arg.split("-")[0]))
    raise KeyError(name)


C_PATTERNS = ("edges", "dead_chunk", "all_dead", "total_255", "total_256", "total_257", "one_long")


def names_a(): return [f"A-{layout}-{c}" for layout in ("single", "spread") for c in A_COLUMNS]
def names_b(): return ["B-few", "B-limit", "B-limit+1"]
def names_c(): return [f"C-records-{r}" for r in C_RECORDS] + [f"C-{p}" for p in C_PATTERNS]
def names_d(): return ["D-leaves-in-chunk-1", "D-leaves-in-chunk-2"]
def names_e(): return [f"E-{r}-rows" for r in E_ROWS]
def names_w(): return [f"W-{c}-cells" for c in WIDTHS]
def single_names(): return names_a() + names_b() + names_c() + names_d() + names_e() + names_w()
def all_names(): return single_names() + ["F-tables"]


# ---- cases outside the word construction: the union's fold inside a wide group, and sums near 2^20 ----------------------------------
# Their genes are written out letter by letter, so there is no plan_row for them: a RawCase DECLARES every row's distinct columns and
# the rows with more than QJ_LIMIT lookups, and tests/test_query_join_sets_cpu.py holds both against the oracle's dictionary.
@dataclass
class RawCase:
    name: str
    base_genes: list
    query_genes: list
    columns: list                   # per query row: distinct columns
    may_overflow: int               # rows with more than QJ_LIMIT lookups
    note: dict = field(default_factory=dict)

    @property
    def N(self): return len(self.base_genes)
    @property
    def queries(self): return [self.query_genes]

    @functools.cached_property
    def base(self):
        genome_of = np.minimum(np.arange(self.N) * 3 // max(self.N, 3), 2)
        gs = H.as_gene_set(self.base_genes, genome_of, np.full(self.N, -1))
        return gs.residues, gs.offsets, gs.genome_of

    def query(self, q=0):
        off = np.zeros(len(self.query_genes) + 1, np.uint64)
        np.cumsum([len(g) for g in self.query_genes], out=off[1:])
        return np.concatenate(self.query_genes).astype(np.uint8), off

    def union(self, q=0):
        rb, ob_, gb = self.base
        rq, oq = self.query()
        return (np.concatenate([rb, rq]).astype(np.uint8), np.concatenate([ob_, ob_[-1] + oq[1:]]).astype(np.uint64),
                np.concatenate([gb, np.full(len(oq) - 1, 3, np.uint32)]).astype(np.uint32), 3)

    def expected_overflow(self, q=0): return overflow_interval(self.columns)
    def expected_may_overflow(self, q=0): return self.may_overflow


def _b(s: bytes) -> np.ndarray: return np.frombuffer(s, np.uint8).copy()


def _alphabet_gene(extra: bytes = b"") -> np.ndarray:
    """V Q V Q V Q V and, where asked, one more letter at the very END: no window starts with it"""
    return np.r_[_b(b"VQVQVQV"), _b(extra)]


FOLD_WIDE, FOLD_BELOW = 3900, 3000          # members of the group the fold touches: above QJ_LIMIT + QJ_T, below QJ_LIMIT
TOP = bytes([JE.TOP_LETTER]) * K            # YYYYY: the base's largest k-mer
R2 = TOP[:-1] + bytes([JE.COLUMN_SEPARATOR])   # YYYYW: the largest k-mer below it


def case_fold(variant: str, wide: bool) -> RawCase:
    """Q1 of the union (pdl_query.h, head of the file) where the group it changes has W = 3900 members (the HBM tables) or 3000 (LDS).
      "qextra"  W base genes hold YYYYY, the base's largest k-mer (nothing is folded in the base).  The query gene ZACDE is one record
                above it, alone in its rank: the union folds it into the group of YYYYY (QDesc.qextra) — for its own row, one record
                of W + 1 columns, and for the row of the query gene that holds YYYYY.
      "bskip"   one base gene T is YYYYY, alone in its rank: the base folded it into the group of YYYYW, held by W base genes, T in the
                middle of them by gene id.  The query holds YYYYY too, so in the union T is an ordinary group again: the row of the
                query gene that holds YYYYW walks [gs, U) without T (QDesc.bskip) — W columns, not W + 1.
      "bextra"  the same T, and no base k-mer between YYYYY and the fillers.  W query genes hold YYYYW, the query's largest rank, below
                YYYYY and above the base's second: T joins THEIR group (QDesc.bextra) — every row has the W - 1 others and T as columns."""
    W = FOLD_WIDE if wide else FOLD_BELOW
    name = f"G-{variant}-{'wide' if wide else 'below'}"
    sep = _b(b"Q")
    dead = JE.filler(26000, 15)
    if variant == "qextra":
        base = [np.r_[_b(TOP), JE.filler(i, 35)] for i in range(W)] + [_alphabet_gene(b"Z")]
        query = [_b(b"ZACDE"), np.r_[_b(TOP), np.repeat(sep, 5)], dead]
        return RawCase(name, base, query, [W + 1, W + 1, 0], 2 if W + 2 > QJ_LIMIT else 0)
    if variant == "bskip":
        holders = [np.r_[_b(R2), JE.filler(i, 35)] for i in range(W)]
        base = holders[:W // 2] + [_b(TOP)] + holders[W // 2:] + [_alphabet_gene()]
        query = [_b(TOP), np.r_[_b(R2), np.repeat(sep, 5)], dead]
        return RawCase(name, base, query, [1, W, 0], 1 if W + 1 > QJ_LIMIT else 0, note={"T": W // 2})
    if variant == "bextra":
        # (the payload letters in ascending order: the query's fillers bring all of them, and no window of theirs is without a V)
        base = [JE.filler(i, 15) for i in range(3)] + [_b(TOP)] + [JE.filler(4 + i, 15) for i in range(2)] + [JE.PAYLOAD.copy(), _alphabet_gene(b"W")]
        query = [np.r_[_b(R2), JE.filler(22000 + j, 35)] for j in range(W)]
        return RawCase(name, base, query, [W] * W, W, note={"T": 3})
    raise KeyError(variant)


# Large counts: the three 21-bit sums of the packed accumulator (min, the row's count, the column's count: q_walk_row) close to the
# 2^20 the guard allows.  K-rle is quadratic in ONE run (runs stay at 3000), so the sums are made of many runs:
# 50 stretches of a 7-letter unit repeated 2990 times — 350 k-mers, 2990 times each: 1 046 500 k-mers in a gene of 1 046 696.
L_STRETCHES, L_PERIOD, L_REPEATS = 50, 7, 2990
L_SUM = L_STRETCHES * L_PERIOD * L_REPEATS
assert (1 << 20) - 2100 < L_SUM < L_SUM + L_STRETCHES * (K - 1) < GENE_KMERS_GUARD


def _giant(repeats) -> np.ndarray:
    rng = np.random.default_rng(20)
    units = [H.LETTERS[rng.permutation(19)[:L_PERIOD]] for _ in range(L_STRETCHES)]        # (no Y: the top k-mer stays the trailing genes')
    return np.concatenate([H.stretch(u, r, K) for u, r in zip(units, repeats)])


def case_large(overflowing: bool) -> RawCase:
    """The query gene is the giant, every k-mer 2990 times.  Base gene 0 is its twin (the three sums are all L_SUM), base gene 1 holds
    the even stretches 2990 times and the odd ones 1500 times (min and the column's sum differ from the row's), base gene 2 the other
    way round.  `overflowing`: the query gene ends with the k-mer PPPPP, which 3900 more base genes hold: the same three cells are
    then accumulated on the tables in HBM."""
    full = [L_REPEATS] * L_STRETCHES
    half = [L_REPEATS if i % 2 == 0 else 1500 for i in range(L_STRETCHES)]
    flip = [1500 if i % 2 == 0 else L_REPEATS for i in range(L_STRETCHES)]
    base = [_giant(full), _giant(half), _giant(flip)]
    wide = _b(b"PPPPP")
    n_wide = FOLD_WIDE if overflowing else 0
    rng = np.random.default_rng(21)
    base += [np.r_[wide, _b(b"Y"), H.LETTERS[rng.integers(0, 19, 30)]] for _ in range(n_wide)]
    base += [np.r_[_b(TOP), _b(b"Y"), H.LETTERS[rng.integers(0, 19, 30)]] for _ in range(2)]
    query = [np.r_[_giant(full), _b(b"Y"), wide] if overflowing else _giant(full), H.LETTERS[:K - 1].copy()]      # (and a gene shorter than k)
    return RawCase(f"H-large-{'hbm' if overflowing else 'lds'}", base, query, [3 + n_wide, 0], 1 if overflowing else 0)


I_BASE, I_QUERY = QJ_LIMIT - 84, 341         # 3500 base columns: they fit the LDS table; with the 340 other query genes: QJ_LIMIT + QJ_T


def case_query_columns() -> RawCase:
    """The columns that carry a row over the limit are genes of the same query: 3500 base genes and 341 query genes hold PPPPP, each
    with a filler of its own behind it (rows built the way columns are: the windows that run into the filler are shared with other
    holders of the word, never with anybody else) — every query row has 3500 + 340 columns and must leave the LDS table: 341
    overflowing rows, whose tables are laid out for N + 341 columns."""
    word = _b(b"PPPPP")
    base = [np.r_[word, JE.filler(i, 35)] for i in range(I_BASE)]
    base += [np.r_[np.full(K + 1, JE.TOP_LETTER, np.uint8), JE.filler(I_BASE + i, 15)] for i in range(2)]
    query = [np.r_[word, JE.filler(22000 + j, 35)] for j in range(I_QUERY)]
    assert I_BASE <= QJ_LIMIT and I_BASE + I_QUERY - 1 == MUST_LEAVE
    return RawCase("I-query-columns", base, query, [MUST_LEAVE] * I_QUERY, I_QUERY)


@functools.lru_cache(maxsize=None)
def raw_case(name: str) -> RawCase:
    kind, a, b = name.split("-")
    if kind == "I":
        return case_query_columns()
    if kind == "G":
        return case_fold(a, b == "wide")
    if kind == "H":
        return case_large(b == "hbm")
    raise KeyError(name)


def names_g(): return [f"G-{v}-{w}" for v in ("qextra", "bextra", "bskip") for w in ("wide", "below")]
def names_h(): return ["H-large-lds", "H-large-hbm"]
def names_i(): return ["I-query-columns"]
def raw_names(): return names_g() + names_h() + names_i()


# ---- the walk's search, restated -----------------------------------------------------------------------------------------------------
def walk_chunk(sizes, strict: bool = False):
    """q_walk_row over ONE chunk of records with these group sizes (0: a zero-size record): the exclusive scan s_pre and, for every
    lookup t of the chunk, the binary search for "the last record i with s_pre[i] <= t" as the kernel writes it (lo = 0, hi = QJ_T;
    records past the chunk's end have size 0).  strict: the search with `<` instead.  -> [(record, member)] per lookup"""
    sz = np.zeros(QJ_T, np.int64)
    sz[:len(sizes)] = sizes
    pre = np.r_[0, np.cumsum(sz)]
    out = []
    for t in range(int(pre[QJ_T])):
        lo, hi = 0, QJ_T
        while hi - lo > 1:
            m = (lo + hi) >> 1
            if (pre[m] < t) if strict else (pre[m] <= t):
                lo = m
            else:
                hi = m
        out.append((lo, t - int(pre[lo])))
    return out
