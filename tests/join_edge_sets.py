"""Gene sets with PLANTED rows for the join tiers (pandelos_amd/csrc/pdl_join.hip, pdl_join_part.h): rows whose number of ranges,
range lengths, lookup total, distinct columns and heavy lookups are decided before anything runs, so that a row can be put ON a
limit of a table, a staging batch, a walk step or a tier-0 cycle.  Pure numpy, no device.

A planted row is described by its INCIDENCE: for range i, in rank order, the columns that hold that k-mer, each column's count of
it, and the row's own count (`Row`).  `planted_rows` turns one to four such rows into a GeneSet at k = 5:

  words     five letters over the 13-letter payload alphabet A..P: the base-13 numbers i * stride, spread evenly over the 13^5 there
            are.  Distinct, and lexicographic order = rank order = order of i: range i of a row is its i-th smallest word.
  a row     its words joined by a separator letter of its own (Q R S T for rows 0-3) and a tail of separators; a word the row
            holds twice stands twice
  a column  the words it holds (twice where its count is 2), a W behind each, then its filler
  filler    V d0 d1 d2 d3 over and over: the gene id in base 13, lowest digit first.  Every window inside it holds a V and all four
            digits, so it is the gene's alone.  The digits are payload letters; the W behind a column's last word keeps "l l l l V" and
            "l V d0 d1 d2" out of the set, which would be windows of some all-filler gene: a column shares k-mers with columns of its
            row's pool and nothing else, an all-filler gene with nobody.  The length decides the gene's k-mer count: a column of two
            sightings has 14 k-mers — more than 2k, so the filters stay on (pdl_join.hip:522), and few enough for 2 / 14 >= 1 / 2k:
            the reference EMITS the planted row's cell of that column (library.cpp:497-500), and its three sums are compared.  A
            column of a single sighting gets 13 k-mers and, rightly, no cell.  `long_fillers` makes every gene 31 k-mers or longer
            (columns then need four sightings for their cell): the sift threshold of the set is then 4, where the partition tier runs
            its counter form (PT_SIFT_T_MIN); with short fillers it is 2 and the bitmap form runs.
  trailing  two genes that hold YYYYY, the largest k-mer of the set: the reference folds the globally LAST record into the group in
            front of it (library.cpp:300-306; helpers.rank_groups restates it), and the last record is then a member of that group
            already.  Without them the largest k-mers would be a planted row's separator windows and the row would gain a range.

A k-mer that spans a join or runs into a filler holds one of Q R S T V W Y and so is no word; a row's separator is in no other
gene, so its spanning windows make no group: a planted row has the planned ranges and no other.  Columns do share spanning windows
with each other (those that hold the same word, or words with the same outer letters): `describe` measures, for every unplanted
gene, with how many genes it shares a k-mer, and every set declares a bound for it that the CPU tests enforce.

Gene order: the planted rows are the first genes of genome 0 and their columns follow — in mirror mode a row meets only the genes
above it (pdl_join.hip:22-25).  `middle=True` puts the planted rows at the start of genome 1 instead, with half of the columns below
them (for a genome shard set before the build, where rows keep whole groups: the row itself is then a posting of each of its
ranges).  Then padding genes (fillers only: they raise N, and with it the put-aside capacity of the filter tiers, without touching a
planted row), the optional short gene, the trailing genes.

The table of limits restates the kernels' constants; a tier assertion that fails after a limit has moved says which."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from tests import helpers as H

K = 5
PAYLOAD = np.frombuffer(b"ACDEFGHIKLMNP", dtype=np.uint8)
ROW_SEPARATORS = b"QRST"
COLUMN_SEPARATOR, FILLER_MARK, TOP_LETTER = ord("W"), ord("V"), ord("Y")
WORDS = len(PAYLOAD) ** K
MAX_PLANTED = len(ROW_SEPARATORS)


# ---- the limits ----------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Form:
    """One instance of k_join_lds as the host launches it (JOIN_KERNELS, pdl_join.hip:1664-1671)"""
    name: str
    options: tuple                 # pdl_set_option pairs that make this instance the first tier every row comes to
    ht_bits: int                   # JoinCfg::HT = 1 << ht_bits                                 pdl_join.hip:172
    threads: int                   # T_
    filtered: bool                 # FILTER
    chunks_per_step: int           # NCH: chunks of 64 lookups a wave maps per step             pdl_join.hip:193
    handed_on: str                 # the pdl_timings counter of the tier behind it

    @property
    def ht(self): return 1 << self.ht_bits
    @property
    def limit(self): return self.ht - self.threads - self.ht // 8                # JoinCfg::LIMIT      pdl_join.hip:173
    @property
    def touch_cap(self): return self.limit + self.threads                        # JoinCfg::TOUCH_CAP  pdl_join.hip:174
    @property
    def rb(self): return (2 if self.filtered else 1) * self.threads              # JoinCfg::RB         pdl_join.hip:175-176
    @property
    def waves(self): return self.threads // 64
    @property
    def bitmap_bits_log2(self): return 15 if self.ht_bits <= 10 else 16          # JoinCfg::BM_BITS_LOG2  pdl_join.hip:179


FORMS = {f.name: f for f in (
    Form("t1_9", (("join_tier1", 9),), 9, 128, True, 4, "tier2_rows"),
    Form("t1_10", (("join_tier1", 10),), 10, 256, True, 4, "tier2_rows"),
    Form("t1_11", (("join_tier1", 11),), 11, 256, True, 8, "tier2_rows"),
    Form("t1_20", (("join_tier1", 20),), 10, 256, False, 4, "tier2_rows"),
    Form("t1_21", (("join_tier1", 21),), 11, 256, False, 4, "tier2_rows"),
    Form("tier2", (("join_tier1", 0),), 13, 1024, False, 4, "overflow_rows"),
    Form("tiny2", (("join_tier1", 0), ("join_tiny_tier2", 1)), 9, 64, False, 4, "overflow_rows"),
)}
# the table as DESIGN.md section 3 prints it: {form: (LIMIT, TOUCH_CAP, RB)} — test_join_edge_sets_cpu holds FORMS against it
LIMITS = {"t1_9": (320, 448, 256), "t1_10": (640, 896, 512), "t1_11": (1536, 1792, 512), "t1_20": (640, 896, 256),
          "t1_21": (1536, 1792, 256), "tier2": (6144, 7168, 1024), "tiny2": (384, 448, 64)}
# tier 0 (pdl_join_part.h)
PT_RB, PT_ROWS, PT_HEAVY_CAP = 960, 4, 64                # :48 ranges per cycle, :49 rows per cycle, :55 listed heavy lookups per cycle
PT_LMAX = {256: 4096, 512: 8192}                         # :101 lookups per cycle = PT_KPT (:54, 16) * threads of the form (:46-47)
PT_HT = 1024                                             # :67
PT_PART = {1: 1024, 2: 512, 3: 256, 4: 256}              # :266 a row's part of the table in a cycle of 1, 2, 3-4 rows
PT_PART_KEYS = {n: 3 * s // 4 for n, s in PT_PART.items()}      # :267 ... which takes keys until three quarters full
PT_SIFT_T_MIN = 4                                        # :65 below it the bitmap form of the kernel runs
TIER3_COLUMNS = 600                                      # a row for the HBM kernel behind the tiny tier 2: more columns than its 384


def defer_cap(n_genes: int, lookups_per_row: int = 0) -> int:
    """entries of a workgroup's put-aside list (pdl_join.hip:1948); a wave's part is defer_cap // waves (:525)"""
    return min(max(4 * lookups_per_row, 8192), 1 << 18, n_genes + 64)


def bitmap_bit(form: Form, gene) -> np.ndarray:
    """the "seen once" bit of a column in a filter form (pdl_join.hip:551)"""
    return ((np.asarray(gene, np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xffffffff)) >> np.uint64(32 - form.bitmap_bits_log2)


# ---- incidence -----------------------------------------------------------------------------------------------------------------
@dataclass
class Row:
    """A planted row: ranges in rank order.  cols[i]: ascending local column ids of range i; ccnt[i]: their counts of the k-mer
    (None: all 1); own[i]: the row's own count (1 or 2)."""
    cols: list
    ccnt: list = None
    own: list = None

    def __post_init__(self):
        self.cols = [np.asarray(c, np.int64) for c in self.cols]
        self.ccnt = [np.ones(len(c), np.int64) for c in self.cols] if self.ccnt is None else [np.asarray(c, np.int64) for c in self.ccnt]
        self.own = np.ones(len(self.cols), np.int64) if self.own is None else np.asarray(self.own, np.int64)
        assert all(len(c) > 0 and np.all(np.diff(c) > 0) for c in self.cols) and all(len(a) == len(b) for a, b in zip(self.cols, self.ccnt))

    @property
    def lens(self): return np.asarray([len(c) for c in self.cols], np.int64)
    @property
    def nr(self): return len(self.cols)
    @property
    def lookups(self): return int(self.lens.sum())
    @property
    def columns(self): return np.unique(np.concatenate(self.cols))
    @property
    def heavy(self):
        """per lookup, in walk order: a count >= 2 on either side"""
        return np.concatenate([(cc >= 2) | (o >= 2) for cc, o in zip(self.ccnt, self.own)])


def cyclic(lens, pool: int, first: int = 0, heavy: float = 0.0, seed: int = 0) -> Row:
    """Ranges of the given lengths over columns first .. first + pool - 1, dealt round: range i takes the next lens[i] columns
    (mod pool), so a column is sighted floor or ceil of sum(lens) / pool times.  `heavy`: that share of the lookups, about, has a
    count of 2 — every twentieth short range is one the row holds twice, and postings picked by `seed` hold the word twice."""
    lens = np.asarray(lens, np.int64)
    assert lens.min() >= 1 and lens.max() <= pool
    at, cols = 0, []
    for n in lens.tolist():
        cols.append(first + np.sort((at + np.arange(n)) % pool))
        at = (at + n) % pool
    rng = np.random.default_rng(seed)
    own = np.ones(len(lens), np.int64)
    if heavy > 0:
        own[np.flatnonzero(lens <= 8)[::20]] = 2
    ccnt = [np.where(rng.random(n) < heavy, 2, 1) for n in lens.tolist()]
    return Row(cols, ccnt, own)


def even_lens(nr: int, lookups: int) -> np.ndarray:
    """nr range lengths, as even as can be, that add up to `lookups`"""
    assert 1 <= nr <= lookups
    return (lookups // nr + (np.arange(nr) < lookups % nr)).astype(np.int64)


def many_short(columns: int) -> Row:
    """lengths 1, 2, ..., 8, 1, ... dealt round twice over: every column has exactly two sightings"""
    lens, left, i = [], 2 * columns, 0
    while left:
        lens.append(min(left, 1 + i % 8, columns)); left -= lens[-1]; i += 1
    return cyclic(lens, columns)


def few_long(columns: int) -> Row:
    """six ranges: three share the columns out between them, and three more do it again"""
    return cyclic(np.tile(even_lens(3, columns), 2), columns)


def spread(columns: int, m: int) -> Row:
    """range i holds m new columns and the m new ones of range i - 1: every column has exactly two sightings, in two ranges next
    to each other, and first sightings are even along the lookup stream"""
    blocks = [np.arange(b, min(b + m, columns)) for b in range(0, columns, m)]
    return Row([blocks[0]] + [np.r_[blocks[i - 1], blocks[i]] for i in range(1, len(blocks))] + [blocks[-1]])


def front_loaded(columns: int, m: int, first: int = 0) -> Row:
    """all first sightings, then all second sightings, in ranges of m"""
    blocks = [first + np.arange(b, min(b + m, columns)) for b in range(0, columns, m)]
    return Row(blocks + blocks)


def concat(rows) -> Row:
    return Row([c for r in rows for c in r.cols], [c for r in rows for c in r.ccnt], np.concatenate([r.own for r in rows]))


# ---- the builder ---------------------------------------------------------------------------------------------------------------
def word(i: int) -> np.ndarray:
    return PAYLOAD[[i // 13 ** 4, i // 13 ** 3 % 13, i // 169 % 13, i // 13 % 13, i % 13]]


def filler(gene: int, chars: int) -> np.ndarray:
    assert gene < 13 ** 4
    unit = np.r_[FILLER_MARK, PAYLOAD[[gene % 13, gene // 13 % 13, gene // 169 % 13, gene // 2197 % 13]]].astype(np.uint8)
    return np.resize(unit, chars)


@dataclass
class Planted:
    """What planted_rows built: the set, the planted rows' gene ids and incidence, where local column c lives"""
    gs: object
    rows: list                     # [Row]
    row_genes: list                # gene id of each planted row
    column_gene: np.ndarray        # gene id of local column c
    middle: bool
    short_gene: int                # k-mers of the short gene planted on purpose (0: none)
    unplanted_partners: int = 64   # bound on the genes an unplanted gene shares a k-mer with (set by the case, enforced by the CPU tests)
    note: dict = field(default_factory=dict)             # what a case wants to tell its test (predictions made from the incidence)


def planted_rows(k: int, rows, padding: int = 0, middle: bool = False, short_gene: int = 0, columns: int = None, long_fillers: bool = False) -> Planted:
    """`rows`: one to four Row over shared local column ids 0 .. columns - 1 (default: the largest id in use + 1; a column no row
    names is one more padding gene, in the columns' place).  `short_gene`: k-mers of one extra gene that shares nothing
    (<= 2k: filters and tier 0 switch off for the whole set; 5k: the partition tier runs its bitmap form)."""
    assert k == K and 1 <= len(rows) <= MAX_PLANTED
    n_pl = len(rows)
    n_col = max(max(int(r.columns.max()) for r in rows) + 1, columns or 0)
    total_ranges = sum(r.nr for r in rows)
    stride = WORDS // total_ranges
    assert stride >= 1
    stride -= stride > 1 and stride % 13 == 0             # (the last letters vary from word to word)
    ids = np.arange(total_ranges) * stride                # row after row: disjoint word sets
    n_before = max(n_col // 2, 1) if middle else 0        # columns below the planted rows
    column_gene = np.where(np.arange(n_col) < n_before, np.arange(n_col), np.arange(n_col) + n_pl)
    row_genes = [n_before + i for i in range(n_pl)]
    held = [[] for _ in range(n_col)]                     # per column: the words it holds, in rank order, twice where its count is 2
    genes, at = {}, 0
    for i, r in enumerate(rows):
        s = np.array([ROW_SEPARATORS[i]], np.uint8)
        parts = []
        for j in range(r.nr):
            w = int(ids[at + j])
            parts += [word(w), s] * int(r.own[j])
            for c, cc in zip(r.cols[j].tolist(), r.ccnt[j].tolist()):
                held[c] += [w] * cc
        at += r.nr
        genes[row_genes[i]] = np.concatenate(parts + [np.repeat(s, 40)])
    sep = np.array([COLUMN_SEPARATOR], np.uint8)
    pad_chars = 35 if long_fillers else 15                # a gene that is all filler: 31 k-mers, or 11
    for c in range(n_col):
        g = int(column_gene[c])
        if not held[c]:
            genes[g] = filler(g, pad_chars); continue
        assert len(held[c]) >= (4 if long_fillers else 1), "with long fillers a column needs four sightings for its cell"
        parts = []
        for w in held[c]:
            parts += [word(w), sep]
        # 6 * words + 11 k-mers with long fillers; else 14 for two words, 20 for three ... and 13 for a single one (no cell, rightly)
        genes[g] = np.concatenate(parts + [filler(g, 15 if long_fillers else 11 if len(held[c]) == 1 else 6)])
    n = n_pl + n_col
    tail = [filler(n + i, pad_chars) for i in range(padding)]
    if short_gene:
        tail.append(filler(n + len(tail), short_gene + K - 1))
    for i in range(2):
        tail.append(np.r_[np.full(K + 1, TOP_LETTER, np.uint8), filler(n + len(tail), pad_chars)])
    seqs = [genes[g] for g in range(n)] + tail
    total = len(seqs)
    idx = np.arange(total)
    if middle:                                            # genome 1 opens with the planted rows
        genome_of = np.where(idx < n_before, 0, np.where(idx < n_before + n_pl + (n_col - n_before + 1) // 2, 1, 2))
    else:
        genome_of = np.minimum(idx * 3 // max(n, 3), 2)   # three genomes; what follows the columns is in the last
        genome_of[:n_pl] = 0
    gs = H.as_gene_set(seqs, genome_of, np.full(total, -1))
    return Planted(gs, list(rows), row_genes, column_gene, middle, short_gene)


# ---- what a set IS, from the oracle's dictionary ----------------------------------------------------------------------------------
def partner_counts(r, gid, start, size, n: int) -> np.ndarray:
    """per gene: the number of OTHER genes it shares a k-mer with (a rank group of the reference's scan), by bit rows"""
    nb = (n + 7) // 8
    bits = np.zeros((n, nb), np.uint8)
    seq = r["seq"].astype(np.int64)
    groups = np.flatnonzero(size >= 2)
    for s in np.unique(size[groups]).tolist():
        gsel = groups[size[groups] == s]
        mem = seq[start[gsel][:, None] + np.arange(s)]                    # [groups of this size][members]
        if s <= 12:
            for i in range(s):
                for j in range(s):
                    if i != j:
                        np.bitwise_or.at(bits, (mem[:, i], mem[:, j] >> 3), (1 << (mem[:, j] & 7)).astype(np.uint8))
        else:
            for row in np.unique(mem, axis=0):
                mask = np.zeros(nb, np.uint8)
                np.bitwise_or.at(mask, row >> 3, (1 << (row & 7)).astype(np.uint8))
                bits[row] |= mask
    me = np.arange(n)
    bits[me, me >> 3] &= ~(1 << (me & 7)).astype(np.uint8)
    pop = np.array([bin(i).count("1") for i in range(256)], np.int64)
    return pop[bits].sum(axis=1)


def describe(case: H.OracleCase, pl: Planted):
    """-> {"rows": [per planted row: lens, cols (gene ids per range), heavy per lookup, own counts], "partners": per gene,
    "fold": the genes of the last group of the reference's scan — the one the folded record joins} from the oracle's dictionary
    alone.  A row's ranges are its records in groups of two or more, in rank order; in the default order it meets the members above
    it, with middle=True (a shard: whole groups) all the others."""
    r, gid, start, size = H.rank_groups(case.dictionary)
    out = {"rows": []}
    for g in pl.row_genes:
        lens, cols, heavy, own = [], [], [], []
        for i in np.flatnonzero(r["seq"] == g).tolist():
            lo, hi = int(start[gid[i]]), int(start[gid[i]] + size[gid[i]])
            others = np.r_[np.arange(lo, i), np.arange(i + 1, hi)] if pl.middle else np.arange(i + 1, hi)
            if len(others) == 0:
                continue
            lens.append(len(others)); cols.append(r["seq"][others].astype(np.int64)); own.append(int(r["count"][i]))
            heavy.append((r["count"][others] >= 2) | (r["count"][i] >= 2))
        out["rows"].append({"lens": np.asarray(lens, np.int64), "cols": cols, "own": np.asarray(own, np.int64),
                            "heavy": np.concatenate(heavy) if heavy else np.zeros(0, bool)})
    out["partners"] = partner_counts(r, gid, start, size, case.gs.genes)
    out["fold"] = sorted(set(r["seq"][start[-1]:].tolist()))
    return out


# ---- the sets of tests/test_gpu_join_edges.py ---------------------------------------------------------------------------------------
# A set is named by a tuple; `planted(name)` builds it, `case(name)` adds the oracle's answer.  Both are made once and never changed.
A_FORMS = ("t1_20", "t1_21", "tier2", "tiny2")
B_FORMS = ("t1_9", "t1_10", "t1_11")
C_FORMS = ("t1_10", "t1_11", "t1_20", "tier2", "tiny2")
D_FORMS = ("t1_10", "t1_11", "t1_21", "tier2", "tiny2", "tier3")
D_PATTERNS = ("700x1", "40x64", "40x63", "40x65", "12x256", "6x512", "255_257", "1_long", "long_ones", "ones_long", "3x70", "mix",
              "63x4_3_1", "63x8_7_1", "64x4", "64x8")
F_FORMS = ("t1_10", "tier2")


def sweep_k(form: Form):
    return [form.limit - 1, form.limit, form.limit + 1, form.touch_cap, form.touch_cap + 1]


def d_pool(form_name: str) -> int:
    return TIER3_COLUMNS if form_name == "tier3" else FORMS[form_name].limit - 1


def d_lens(pattern: str, pool: int):
    """range lengths of a walk pattern (section D), in rank order; None where the pool has no room for its longest range"""
    long = min(4100, pool)
    lens = {"700x1": [1] * 700, "40x64": [64] * 40, "40x63": [63] * 40, "40x65": [65] * 40, "12x256": [256] * 12, "6x512": [512] * 6,
            "255_257": [255, 257] * 6, "1_long": [1, long] * 3, "long_ones": [long] + [1] * 200, "ones_long": [1] * 200 + [long],
            "3x70": [70] * 3,
            # a step of 4 (8) chunks whose 64th range start is its LAST lookup and whose 65th opens the next step: one read of 64
            # starts falls one short of the step's end (readlane(vw, 63) == f_hi - 1), and the per-chunk path has to take over
            "63x4_3_1": ([4] * 63 + [3, 1]) * 8, "63x8_7_1": ([8] * 63 + [7, 1]) * 8,
            # ... and whose 64th following range opens the next step: readlane(vw, 63) == f_hi, the one-read path at equality
            "64x4": [4] * 512, "64x8": [8] * 512}.get(pattern)
    if lens is None:
        lens = np.random.default_rng(11).choice([1, 2, 3, 5, 64, 200], 400).tolist()
    return lens if max(lens) <= pool and (pool != TIER3_COLUMNS or sum(lens) >= pool) else None


def exactly_full(form: Form):
    """Section B, "exactly full": a row of LIMIT - 1 columns of two sightings whose FIRST wave files a known number of first sightings.
    Every wave walks a segment of seg = 64 * ceil(ceil(L / 64) / waves) lookups (pdl_join.hip:349-350), and a column's bit goes to
    the wave that sights it first IN TIME — so both sightings of a column lie in one wave's segment: the row is one front-loaded
    chain per wave, each chain a segment long.  Wave 0's chain opens with `singles` columns of a single sighting: they raise its
    count over what the smallest set gives every wave room for.  A single must not get a key (it would make LIMIT keys or more):
    singles are picked among ids whose bit no other column of the row shares.
    -> (Row, columns, first sightings wave 0 files at least, at most)"""
    nw, k2 = form.waves, form.limit - 1
    singles = 64 if nw >= 4 else 192
    seg = -(-(-(-(2 * k2 + singles) // 64)) // nw) * 64
    x0 = (seg - singles) // 2
    assert singles + 2 * x0 == seg and 2 * (k2 - x0) > (nw - 2) * seg and 2 * (k2 - x0) <= (nw - 1) * seg
    bits2 = bitmap_bit(form, 1 + np.arange(k2))           # (one planted row: local column c is gene 1 + c)
    taken, pick, c = set(bits2.tolist()), [], k2
    while len(pick) < singles:
        b = int(bitmap_bit(form, 1 + c))
        if b not in taken:
            taken.add(b); pick.append(c)
        c += 1
    chains = [concat([Row([np.asarray(pick[i:i + 8]) for i in range(0, singles, 8)]), front_loaded(x0, 8)])]
    at = x0
    for w in range(1, nw):
        n = min(seg // 2, k2 - at)
        chains.append(front_loaded(n, 8, first=at)); at += n
    assert at == k2
    row = concat(chains)
    assert row.lookups == 2 * k2 + singles and -(-(-(-row.lookups // 64)) // nw) * 64 == seg
    mine, others = bits2[:x0], set(bits2[x0:].tolist())
    distinct = len(set(mine.tolist()))
    contested = len(set(mine.tolist()) & others)          # another wave may set these first
    return row, c, singles + distinct - contested, singles + distinct


def full_paddings(form: Form):
    """the eight paddings of the "exactly full" sweep: a wave's part of the put-aside list is (N + 64) // waves entries (while
    N + 64 < 8192), so it moves by one entry per `waves` padding genes — eight parts in a row around the predicted count"""
    row, columns, lo, hi = exactly_full(form)
    base = 1 + columns + 2                                # genes without padding
    return [form.waves * (hi - 4 + i) - 64 - base for i in range(8)]


@functools.lru_cache(maxsize=None)
def planted(name) -> Planted:
    sect = name[0]
    if sect in ("A", "FA"):                               # (section, form, layout, columns)
        _, fname, layout, k = name
        form = FORMS[fname]
        if form.filtered:                                 # (F repeats the sweep on a filter form: B's layout, named "spread")
            pl = planted_rows(K, [spread(k, 4)], padding=k + 64, middle=sect == "FA")
        else:
            pl = planted_rows(K, [many_short(k) if layout == "short" else few_long(k)], middle=sect == "FA")
            if layout == "long":                          # a column meets the others of its third of the columns
                pl.unplanted_partners = -(-k // 3) + 64
        return pl
    if sect == "B":                                       # (B, form, kind, ...)
        _, fname, kind, arg = name
        form = FORMS[fname]
        if kind == "spread":                              # N >= 2K + 64: every wave's part of the put-aside list has room
            return planted_rows(K, [spread(arg, 4)], padding=arg + 64)
        if kind == "unfiltered":                          # one gene of 2k k-mers: every lookup gets its key at once
            return planted_rows(K, [spread(arg, 4)], padding=arg + 64, short_gene=2 * K)
        if kind == "front":
            return planted_rows(K, [front_loaded(form.limit - 1, 8 if fname == "t1_11" else 4)])
        row, columns, lo, hi = exactly_full(form)
        pl = planted_rows(K, [row], padding=full_paddings(form)[arg], columns=columns)
        pl.note = {"filed_lo": lo, "filed_hi": hi, "part": defer_cap(pl.gs.genes) // form.waves}
        return pl
    if sect == "C":                                       # (C, form, ranges)
        _, fname, nr = name
        form = FORMS[fname]
        lens = 1 + np.arange(nr) % 2
        pool = min(form.limit - 1, int(lens.sum()) // 2)
        return planted_rows(K, [cyclic(lens, pool)], padding=form.waves * pool if form.filtered else 0)
    if sect in ("D", "FD"):                               # (section, form, pattern, heavy)
        _, fname, pattern, heavy = name
        pool = d_pool(fname)
        lens = d_lens(pattern, pool)
        if fname != "tier3":                              # (the HBM kernel's row keeps its 600 columns, sighted once where the pattern is short)
            pool = max(min(pool, sum(lens) // 2), max(lens))      # two sightings a column where the pattern has the lookups for it
        filtered = fname != "tier3" and FORMS[fname].filtered
        pl = planted_rows(K, [cyclic(lens, pool, heavy=0.1 if heavy else 0.0, seed=len(pattern))], middle=sect == "FD",
                          padding=max(0, FORMS[fname].waves * pool + 64 - pool) if filtered else 0)
        pl.unplanted_partners = pool                      # the columns share the row's words among themselves: the pool's other columns and the row
        return pl
    if sect == "E":                                       # (E, kind, a, b, short gene)
        _, kind, a, b, short = name
        first, rows = 0, []

        def row(nr, lookups, pool, heavy_postings=0):
            nonlocal first
            r = cyclic(even_lens(nr, lookups), pool, first=first)
            for i in range(heavy_postings):               # the first posting of every fourth range holds the word twice
                r.ccnt[4 * i][0] = 2
            first += pool
            rows.append(r)
        if kind == "ranges":                              # a: rows, b: ranges of the last one; the others have 240
            for i in range(a):
                nr = b if i == a - 1 else 240
                row(nr, 2 * nr, nr // 2)
        elif kind == "lookups":                           # a: rows, b: lookups of the last one; the others have 1024
            for i in range(a):
                n = b if i == a - 1 else 1024
                # alone, 512 columns (a cycle of one row takes 768 keys); four together, 128 each, eight sightings a column: a row's
                # part of a 3-4 row cycle takes 192 keys, and a cycle whose part overflows is thrown away and its rows run one by one
                row(min(512, n // 8), n, 512 if a == 1 else 128)
        elif kind == "columns":                           # a: rows, b: columns of each, four sightings a column; together 960 ranges
            for i in range(a):
                row(PT_RB // a, 4 * b, b)
        elif kind == "heavy":                             # one row alone in its cycle (960 ranges), b heavy lookups
            row(PT_RB, 2 * PT_RB, PT_RB // 2, heavy_postings=b)
        pl = planted_rows(K, rows, long_fillers=True, short_gene=5 * K if short else 0)
        pl.unplanted_partners = 64
        return pl
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name) -> H.OracleCase:
    return H.OracleCase(planted(name).gs, K)


def names_a(): return [("A", f, layout, k) for f in A_FORMS for layout in ("short", "long") for k in sweep_k(FORMS[f])]
def names_b_spread(): return [("B", f, "spread", k) for f in B_FORMS for k in sweep_k(FORMS[f])]
def names_b_unfiltered(): return [("B", "t1_10", "unfiltered", k) for k in (FORMS["t1_10"].limit - 1, FORMS["t1_10"].limit + 1)]
def names_b_front(): return [("B", f, "front", 0) for f in B_FORMS]
def names_b_full(): return [("B", f, "full", i) for f in B_FORMS for i in range(8)]
def names_c(): return [("C", f, nr) for f in C_FORMS for rb in [FORMS[f].rb] for nr in (rb - 1, rb, rb + 1, 2 * rb, 2 * rb + 1)]
def names_d(): return [("D", f, p, h) for f in D_FORMS for p in D_PATTERNS for h in (0, 1) if d_lens(p, d_pool(f)) is not None]


E_KINDS = ([("ranges", 4, 240), ("ranges", 4, 241), ("ranges", 1, 960), ("ranges", 1, 961),
            ("lookups", 4, 1024), ("lookups", 4, 1025), ("lookups", 1, 4096), ("lookups", 1, 4097), ("lookups", 1, 8192), ("lookups", 1, 8193)]
           + [("columns", 1, c) for c in (767, 768, 769)] + [("columns", 2, c) for c in (383, 384, 385)] + [("columns", 4, c) for c in (191, 192, 193)]
           + [("heavy", 1, h) for h in (63, 64, 65)])


def names_e(): return [("E",) + kind + (0,) for kind in E_KINDS] + [("E",) + kind + (1,) for kind in E_KINDS[:4]]


def names_f():
    out = []
    for f in F_FORMS:
        # with a shard the row is a posting of its own ranges and takes a key: LIMIT - 2 and LIMIT columns make LIMIT - 1 and LIMIT + 1 keys
        out += [("FA", f, layout, FORMS[f].limit - 1 + d) for layout in (("spread",) if FORMS[f].filtered else ("short", "long")) for d in (-1, 1)]
        out += [("FD", f, p, 0) for p in D_PATTERNS[:4]]
    return out


def all_names():
    return names_a() + names_b_spread() + names_b_unfiltered() + names_b_front() + names_b_full() + names_c() + names_d() + names_e() + names_f()


def ident(name) -> str:
    return "-".join(str(x) for x in name)
