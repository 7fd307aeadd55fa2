"""Case tables, seeded input generators and numpy references for the three generic device primitives, driven through the test
hooks of pandelos_amd/csrc/pdl_hooks.hip:

  scan      scan_and_apply (pdl_scan.h), three launches or one (option onepass_scan)
  offsets   pdl_radix_offsets (pdl_sort.hip), one launch per pass (option lean_radix) or the three-launch scan over the table
  sort      pdl_sort_pairs (pdl_sort.hip)
  merge     pdl_merge_streams (pdl_append.h)

Every result is an integer: the references are exact.  The sizes are chosen by the constants below, each of which switches a
code path; tests/test_primitive_cases_cpu.py asserts without a device that every case lies on the side of its constant its name
says and holds the references against a second, naive formulation; tests/test_gpu_primitives.py runs the cases."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np

# ---- the regime constants (one place; the kernels' names for them beside) --------------------------------------------------------
SCAN_TILE = 2048              # SCAN_TILE = MG_TILE: elements of a scan tile, outputs of a merge tile
SCAN_INLINE_TILES = 1024      # SCAN_INLINE_TILES: up to here k_scan_apply adds up the tile sums itself, above: k_scan_tile_scan
SCAN_ONE_TRIP_TILES = 16384   # 1024 * TS_ITEMS: up to here k_scan_tile_scan is one block scan, above: trips of 1024 with a carry
RADIX_TILE = 4096             # PDL_RADIX_TILE = RO_TRIP: elements of a radix tile; entries of a row k_rs_offsets takes per trip
RO_MAX_TILES = 65536          # RO_MAX_TILES: longer rows take the three-launch scan under lean_radix too
LB_CHUNK = 64                 # LB_CHUNK: tiles per chunk of the one-launch scan's look-back
SCAN_CARRY_TRIP = 1024        # tile sums per trip of the carry loop
MG_ITEMS = 8                  # outputs per thread of a merge tile: the thread diagonals
RADIX_BINS = 256

POISON32 = 0xFFFFFFFF
POISON64 = 0xFFFFFFFFFFFFFFFF


def tiles_of(n: int, tile: int) -> int:
    return (n + tile - 1) // tile


# ---- scan ----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ScanCase:
    name: str
    n_bound: int
    kind: str                       # bits | small | max | zero | last_one
    d_n: Optional[int] = None       # the count on the device (None: the host's n_bound counts)
    seed: int = 0

    @property
    def count(self) -> int:
        return self.n_bound if self.d_n is None else min(self.d_n, self.n_bound)


SCAN_N = (1, 255, 256, 257, 2047, 2048, 2049,
          SCAN_INLINE_TILES * SCAN_TILE, SCAN_INLINE_TILES * SCAN_TILE + 1,
          SCAN_ONE_TRIP_TILES * SCAN_TILE, SCAN_ONE_TRIP_TILES * SCAN_TILE + 1,
          (SCAN_ONE_TRIP_TILES + 2 * SCAN_CARRY_TRIP + 5) * SCAN_TILE - 3)
SCAN_SIZE_CASES = tuple(ScanCase(f"n{n}_{kind}", n, kind, seed=i) for i, n in enumerate(SCAN_N) for kind in ("bits", "small"))
SCAN_NEAR_WRAP = ScanCase("near_wrap", (1 << 22) + 5, "max")
SCAN_EDGE_CASES = (SCAN_NEAR_WRAP, ScanCase("all_zero", 5 * SCAN_TILE + 77, "zero"), ScanCase("last_one", 3 * SCAN_TILE + 1, "last_one"),
                   ScanCase("last_one_long", (SCAN_INLINE_TILES + 2) * SCAN_TILE, "last_one"))
SCAN_BOUND_TILES = (5, SCAN_INLINE_TILES + 6)


def _device_counts(bound):
    return (0, 1, SCAN_TILE, bound - 1, bound)


SCAN_COUNT_CASES = tuple(ScanCase(f"bound{t}tiles_dn{dn}", t * SCAN_TILE - 9, "small", d_n=dn, seed=100 + t)
                         for t in SCAN_BOUND_TILES for dn in _device_counts(t * SCAN_TILE - 9))
ONEPASS_TILES = (1, 63, 64, 65, 128, 129, 4096, 4097, 16385)
ONEPASS_CASES = tuple(ScanCase(f"onepass_{t}tiles", t * SCAN_TILE - 3, "small" if t % 2 else "bits", seed=200 + t) for t in ONEPASS_TILES)
ONEPASS_COUNT_CASES = (ScanCase("onepass_129tiles_dn65tiles", 129 * SCAN_TILE, "small", d_n=64 * SCAN_TILE + 1, seed=230),
                       ScanCase("onepass_129tiles_dn0", 129 * SCAN_TILE, "small", d_n=0, seed=231))
ONEPASS_SEQUENCE_TILES = (4097, 65, 16385, 1, 4097)
ONEPASS_SEQUENCE = tuple(ScanCase(f"onepass_seq{i}_{t}tiles", t * SCAN_TILE - 1 - i, "bits" if i % 2 else "small", seed=300 + i)
                         for i, t in enumerate(ONEPASS_SEQUENCE_TILES))
ALL_SCAN_CASES = SCAN_SIZE_CASES + SCAN_EDGE_CASES + SCAN_COUNT_CASES + ONEPASS_CASES + ONEPASS_COUNT_CASES + ONEPASS_SEQUENCE


def scan_flags(case: ScanCase) -> np.ndarray:
    """u32 [n_bound].  `small`: 0..1023, thinned out on long inputs so that the total stays below 2^32 (mean 511.5: dense up to 4 M)."""
    n = case.n_bound
    rng = np.random.default_rng(0x5CA0 + case.seed)
    if case.kind == "bits":
        return rng.integers(0, 2, n, dtype=np.uint32)
    if case.kind == "small":
        f = rng.integers(0, 1024, n, dtype=np.uint32)
        if n > (1 << 22):
            f[rng.random(n, dtype=np.float32) >= np.float32((1 << 21) / n)] = 0      # about 2 M survivors: a total near 2^30
        return f
    if case.kind == "max":
        return np.full(n, 1023, dtype=np.uint32)
    f = np.zeros(n, dtype=np.uint32)
    if case.kind == "last_one":
        f[-1] = 1
    else:
        assert case.kind == "zero"
    return f


def scan_reference(flags: np.ndarray, count: int):
    """-> (exclusive prefix u32 [count], total as a Python int) over flags[0 .. count)"""
    f = flags[:count].astype(np.uint64)
    inc = np.cumsum(f, dtype=np.uint64)
    total = int(inc[-1]) if count else 0
    return (inc - f).astype(np.uint32), total


# ---- offsets -------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class OffsetsCase:
    name: str
    n_tiles: int
    zero_suffix: int                # tiles at the end that hold nothing in any row (what a device-side count leaves)


OFFSETS_TILES = (1, 2, RADIX_TILE - 1, RADIX_TILE, RADIX_TILE + 1, 2 * RADIX_TILE, 2 * RADIX_TILE + 1, RO_MAX_TILES, RO_MAX_TILES + 1)
OFFSETS_CASES = tuple(OffsetsCase(f"{t}tiles", t, t // 3) for t in OFFSETS_TILES)


def offsets_counts(case: OffsetsCase) -> np.ndarray:
    """u32 [256][n_tiles]: a tile's counts add up to at most 4096; every seventh tile holds one digit only, 4096 times"""
    rng = np.random.default_rng(0x0FF5 + case.n_tiles)
    t = case.n_tiles
    counts = rng.integers(0, RADIX_TILE // RADIX_BINS + 1, (RADIX_BINS, t), dtype=np.uint32)
    full = np.arange(0, t, 7)
    counts[:, full] = 0
    counts[rng.integers(0, RADIX_BINS, len(full)), full] = RADIX_TILE
    if case.zero_suffix:
        counts[:, t - case.zero_suffix:] = 0
    return counts


def offsets_reference(counts: np.ndarray, lean: bool):
    """lean -> (each row's exclusive prefix [256][t], the rows' sums [256]); else (the exclusive prefix over the table in
    digit-major order [256][t], the total)"""
    c = counts.astype(np.uint64)
    if lean:
        inc = np.cumsum(c, axis=1, dtype=np.uint64)
        return (inc - c).astype(np.uint32), c.sum(axis=1).astype(np.uint32)
    inc = np.cumsum(c.reshape(-1), dtype=np.uint64)
    return (inc - c.reshape(-1)).astype(np.uint32).reshape(c.shape), int(c.sum())


def offsets_lean_expected(n_tiles: int, lean_radix: int, onepass_scan: int) -> bool:
    return bool(lean_radix) and not onepass_scan and n_tiles <= RO_MAX_TILES


# ---- sort ----------------------------------------------------------------------------------------------------------------------
WIDTHS = ((4, 4), (8, 4), (4, 8))


@dataclass(frozen=True)
class SortCase:
    name: str
    key_bytes: int
    val_bytes: int
    n: int                          # the bound: elements of the input, tiles of the grids
    end_bit: int
    below: bool = False             # keys_below_end_bit
    begin_bit: int = 0
    iota: bool = False
    pattern: str = "random"         # random | equal | descending | one_differs | tile_digit | round_distinct | high
    d_n: Optional[int] = None
    filed: bool = False             # the first pass's histogram comes from the caller
    seed: int = 0

    @property
    def count(self) -> int:
        return self.n if self.d_n is None else min(self.d_n, self.n)

    @property
    def key_bits(self) -> int:
        return 8 * self.key_bytes


SORT_SMALL_N = (1, 63, 64, 65, 1023, 1025, 4095, 4096, 4097, 8193, 100003)
SORT_BIG_N = (RADIX_TILE * RADIX_TILE, RADIX_TILE * RADIX_TILE + 1, (2 * RADIX_TILE + 1) * RADIX_TILE)
SORT_END_BITS_32 = tuple(range(1, 17)) + (17, 24, 31, 32)
SORT_END_BITS_64 = (33, 40, 63, 64)
SORT_SWEEP_N = 10007
SORT_BOUND_TILES = (3, 9)
SORT_PATTERNS = ("equal", "descending", "one_differs", "tile_digit", "round_distinct")


def _w(kb, vb):
    return f"k{kb}v{vb}"


def sort_size_cases(kb, vb):
    """full-width random keys at every small size; values given for odd positions in the list, counted 0, 1, 2, ... for even ones"""
    return tuple(SortCase(f"{_w(kb, vb)}_n{n}", kb, vb, n, 8 * kb, iota=i % 2 == 0, seed=i) for i, n in enumerate(SORT_SMALL_N))


def sort_end_bit_cases(kb, vb):
    bits = SORT_END_BITS_32 + (SORT_END_BITS_64 if kb == 8 else ())
    out = [SortCase(f"{_w(kb, vb)}_end{e}_{'below' if b else 'above'}", kb, vb, SORT_SWEEP_N, e, below=b, iota=(e + b) % 2 == 0, seed=1000 + e)
           for e in bits for b in (True, False)]
    out.append(SortCase(f"{_w(kb, vb)}_end0_counts_as_1", kb, vb, SORT_SWEEP_N, 0, below=True, seed=1100))
    out.append(SortCase(f"{_w(kb, vb)}_end_past_the_width", kb, vb, SORT_SWEEP_N, 8 * kb + 8, seed=1101))
    return tuple(out)


def sort_begin_bit_cases(kb, vb):
    return tuple(SortCase(f"{_w(kb, vb)}_begin{bb}", kb, vb, SORT_SWEEP_N, 32, begin_bit=bb, below=kb == 4, iota=bb == 8, seed=1200 + bb) for bb in (0, 8, 24))


def sort_pattern_cases(kb, vb):
    out = [SortCase(f"{_w(kb, vb)}_{p}", kb, vb, 3 * RADIX_TILE + 100, 8 * kb if p == "descending" else 16, pattern=p, iota=i % 2 == 1, seed=1300 + i)
           for i, p in enumerate(SORT_PATTERNS)]
    if kb == 8:
        out.append(SortCase(f"{_w(kb, vb)}_high", kb, vb, 2 * RADIX_TILE + 9, 64, pattern="high", seed=1310))
    return tuple(out)


def sort_count_cases(kb, vb):
    out = []
    for t in SORT_BOUND_TILES:
        n = t * RADIX_TILE - 5
        for dn in (0, 1, RADIX_TILE, n - 1, n):
            out.append(SortCase(f"{_w(kb, vb)}_bound{t}tiles_dn{dn}", kb, vb, n, 16, d_n=dn, iota=dn % 2 == 0, seed=1400 + t))
    return tuple(out)


def sort_filed_cases(kb, vb):
    out = []
    for t in SORT_BOUND_TILES:
        n = t * RADIX_TILE - 5
        for dn in (None, RADIX_TILE + 1):
            out.append(SortCase(f"{_w(kb, vb)}_filed_bound{t}tiles_dn{dn}", kb, vb, n, 16, d_n=dn, filed=True, seed=1500 + t))
    return tuple(out)


def sort_big_cases(kb, vb):
    """end_bit 16, keys below it: numpy's stable sort of 16-bit keys is a radix sort"""
    return tuple(SortCase(f"{_w(kb, vb)}_big{n}", kb, vb, n, 16, below=True, iota=True, seed=1600 + i) for i, n in enumerate(SORT_BIG_N))


def all_sort_cases():
    out = []
    for kb, vb in WIDTHS:
        for make in (sort_size_cases, sort_end_bit_cases, sort_begin_bit_cases, sort_pattern_cases, sort_count_cases, sort_filed_cases, sort_big_cases):
            out.extend(make(kb, vb))
    return tuple(out)


def sort_top(case: SortCase) -> int:
    """one past the highest bit the sort orders by"""
    end = min(max(case.end_bit, 1), case.key_bits)
    return end if case.below else min(8 * ((end + 7) // 8), case.key_bits)


@functools.lru_cache(maxsize=2)
def _low16(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(0x50A7 + seed).integers(0, 1 << 16, n, dtype=np.uint16)


def sort_keys(case: SortCase) -> np.ndarray:
    """u32 | u64 [n].  Bits at and above end_bit are random unless the case says the keys lie below it."""
    n, dt = case.n, (np.uint64 if case.key_bytes == 8 else np.uint32)
    rng = np.random.default_rng(0x50A7 + case.seed)
    full = (1 << case.key_bits) - 1
    end = min(max(case.end_bit, 1), case.key_bits)
    if n >= SORT_BIG_N[0]:
        assert case.below and end == 16
        return _low16(n, case.seed).astype(dt)
    rand = rng.integers(0, full, n, dtype=dt, endpoint=True)
    limit = dt((1 << end) - 1) if case.below else dt(full)
    p = case.pattern
    if p == "random":
        keys = rand & limit
    elif p == "equal":
        keys = np.full(n, 0x1234 & int(limit), dtype=dt)
    elif p == "descending":
        keys = (dt(full) - dt(17) * np.arange(n, dtype=dt)).astype(dt)
    elif p == "one_differs":             # one digit of one element is another: the second byte, in the middle of a tile
        keys = np.full(n, 0x3355, dtype=dt)
        keys[RADIX_TILE + 1000] = 0x3255
    elif p == "tile_digit":              # a tile holds one value of the low digit, the digit above it is random
        keys = ((np.arange(n, dtype=dt) // dt(RADIX_TILE)) * dt(85) & dt(0xFF)) | (rand & dt(0xFF00))
    elif p == "round_distinct":          # any 64 consecutive elements differ in both digits (37 and 101 are odd)
        i = np.arange(n, dtype=dt)
        keys = (i * dt(37) & dt(0xFF)) | ((i * dt(101) & dt(0xFF)) << dt(8)) | (rand & ~dt(0xFFFF) & limit)
    else:
        assert p == "high" and case.key_bytes == 8
        keys = rand | dt(1 << 63)
    if case.below:
        keys = keys & limit
    return keys.astype(dt)


def sort_values(case: SortCase) -> np.ndarray:
    """the payloads of a case that brings its own: u32, or u64 above 2^32"""
    rng = np.random.default_rng(0x7A15 + case.seed)
    if case.val_bytes == 8:
        return rng.integers(1 << 32, POISON64 - 1, case.n, dtype=np.uint64)
    return rng.integers(0, POISON32 - 1, case.n, dtype=np.uint32)


def sort_order(keys: np.ndarray, count: int, begin_bit: int, top: int) -> np.ndarray:
    """positions of the counted prefix in the sorted order: stable on bits [begin_bit, top)"""
    k = keys[:count]
    width = top - begin_bit
    digit = (k >> k.dtype.type(begin_bit)) & k.dtype.type((1 << width) - 1)
    if width <= 16:
        digit = digit.astype(np.uint16)
    return np.argsort(digit, kind="stable")


def sort_reference(case: SortCase, keys: np.ndarray, vals: Optional[np.ndarray]):
    """-> (keys, values) of the counted prefix, sorted; vals None: the positions"""
    order = sort_order(keys, case.count, case.begin_bit, sort_top(case))
    vdt = np.uint64 if case.val_bytes == 8 else np.uint32
    return keys[:case.count][order], (order.astype(vdt) if vals is None else vals[:case.count][order])


def sort_first_counts(case: SortCase, keys: np.ndarray) -> np.ndarray:
    """u32 [256][tiles of the bound]: per-tile histograms of the first pass's digit over the counted prefix, zeros behind it"""
    t = tiles_of(case.n, RADIX_TILE)
    digit = ((keys[:case.count] >> keys.dtype.type(case.begin_bit)) & keys.dtype.type(0xFF)).astype(np.int64)
    tile = np.arange(case.count, dtype=np.int64) // RADIX_TILE
    return np.bincount(digit * t + tile, minlength=RADIX_BINS * t).astype(np.uint32).reshape(RADIX_BINS, t)


# ---- merge ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class MergeCase:
    name: str
    key_bytes: int
    kind: str
    na: int = 0
    nb: int = 0
    mask_bits: int = 0              # 0: the whole key
    arg: int = 0
    seed: int = 0

    @property
    def mask(self) -> int:
        return (1 << (self.mask_bits or 8 * self.key_bytes)) - 1


@dataclass
class MergeInput:
    a_keys: np.ndarray
    a_vals: np.ndarray
    b_keys: np.ndarray
    b_vals: np.ndarray
    b_val_add: int
    tie_runs: tuple = ()            # (first, one past the last) output positions of the runs of equal keys the case promises


B_VAL_ADD = (1 << 30) + 12345
MERGE_TOTALS = (1, 2047, 2048, 2049, 3 * SCAN_TILE)
TIE_SHORT = tuple(8 * j + s for j in range(1, 9) for s in (-1, 1))            # 7, 9, 15, 17, ... 63, 65
TIE_LONG = (SCAN_TILE - 1, SCAN_TILE + 1)


def merge_cases(kb):
    out = [MergeCase(f"k{kb}_a_empty_nb{n}", kb, "random", 0, n, seed=n) for n in (1, 5, 2 * SCAN_TILE + 3)]
    out += [MergeCase(f"k{kb}_b_empty_tail{t}", kb, "random", 2 * SCAN_TILE + 4 * 3 + t, 0, seed=10 + t) for t in (1, 2, 3)]
    out += [MergeCase(f"k{kb}_b_empty_na1", kb, "random", 1, 0, seed=14)]
    for tot in MERGE_TOTALS[1:]:
        out.append(MergeCase(f"k{kb}_total{tot}", kb, "random", tot - tot // 3, tot // 3, seed=20 + tot))
    out.append(MergeCase(f"k{kb}_all_equal", kb, "equal", 3 * SCAN_TILE + 5, 2 * SCAN_TILE + 3))
    out.append(MergeCase(f"k{kb}_b_below_a", kb, "b_below", 2 * SCAN_TILE + 11, SCAN_TILE + 7, seed=31))
    out.append(MergeCase(f"k{kb}_b_above_a", kb, "b_above", 2 * SCAN_TILE + 11, SCAN_TILE + 7, seed=32))
    for where, pos in (("first", 0), ("last", SCAN_TILE - 1), ("middle", 1001)):
        out.append(MergeCase(f"k{kb}_one_b_per_tile_{where}", kb, "one_b_per_tile", 5 * SCAN_TILE - 5 + 77, 5, arg=pos))
    out.append(MergeCase(f"k{kb}_tie_runs", kb, "tie_runs"))
    out.append(MergeCase(f"k{kb}_four_keys", kb, "few", 30000, 20000, arg=4, seed=41))
    out.append(MergeCase(f"k{kb}_values_to_the_top", kb, "random", 3000, 2500, seed=42, arg=1))
    if kb == 8:
        out.append(MergeCase("k8_random_5M", 8, "random", 3_000_000, 2_000_000, seed=43))
        out.append(MergeCase("k8_high", 8, "high", 5000, 4000, seed=44))
        out += [MergeCase(f"k8_mask{8 * j}", 8, "masked", 3 * SCAN_TILE + 1 + j, 2 * SCAN_TILE - j, mask_bits=8 * j, seed=50 + j) for j in range(1, 8)]
    else:
        out.append(MergeCase("k4_mask16", 4, "masked", 3 * SCAN_TILE + 1, 2 * SCAN_TILE - 1, mask_bits=16, seed=50))
    return tuple(out)


def all_merge_cases():
    return merge_cases(4) + merge_cases(8)


def _tie_runs(dt):
    """Runs of one key, la elements in a and lb in b (la, lb from 8 j +- 1 and 2048 +- 1), between filler keys that occur once
    (in a): a short run starts la - 3 outputs before a tile boundary — its a-part ends three outputs behind the boundary, its
    b-part follows — a long one 1000 before."""
    a, b, runs, key, pos = [], [], [], 1, 0
    pairs = list(zip(TIE_SHORT, TIE_SHORT[::-1])) + [(TIE_LONG[0], TIE_LONG[1]), (TIE_LONG[1], TIE_LONG[0]), (TIE_LONG[1], TIE_LONG[1])]
    for la, lb in pairs:
        lead = la - 3 if la < SCAN_TILE - 1 else 1000
        fill = (-(pos + lead)) % SCAN_TILE                   # filler up to `lead` outputs before the next tile boundary
        a.extend(range(key, key + fill)); key += fill; pos += fill
        a.extend([key] * la); b.extend([key] * lb)
        runs.append((pos, pos + la + lb)); pos += la + lb; key += 1
    a.extend(range(key, key + 100))
    return np.array(a, dtype=dt), np.array(b, dtype=dt), tuple(runs)


def merge_input(case: MergeCase) -> MergeInput:
    dt = np.uint64 if case.key_bytes == 8 else np.uint32
    bits = 8 * case.key_bytes
    rng = np.random.default_rng(0x3E26 + case.seed + 1000 * case.key_bytes)
    na, nb, runs = case.na, case.nb, ()

    def rand_sorted(n, lo=0, hi=(1 << bits) - 1):
        return np.sort(rng.integers(lo, hi, n, dtype=dt, endpoint=True))

    if case.kind == "random":
        a, b = rand_sorted(na), rand_sorted(nb)
    elif case.kind == "equal":
        a, b = np.full(na, 77, dtype=dt), np.full(nb, 77, dtype=dt)
    elif case.kind == "b_below":
        a, b = rand_sorted(na, 1 << 20, 1 << 21), rand_sorted(nb, 0, (1 << 20) - 1)
    elif case.kind == "b_above":
        a, b = rand_sorted(na, 0, (1 << 20) - 1), rand_sorted(nb, 1 << 20, 1 << 21)
    elif case.kind == "one_b_per_tile":      # a = 2, 4, 6, ...; b's element of tile t follows the t * 2048 + arg - t elements of a before it
        a = (2 * np.arange(na, dtype=dt) + 2).astype(dt)
        t = np.arange(nb, dtype=dt)
        b = (2 * (t * dt(SCAN_TILE) + dt(case.arg) - t) + 1).astype(dt)
    elif case.kind == "tie_runs":
        a, b, runs = _tie_runs(dt)
    elif case.kind == "few":
        vals = np.array([3, 1 << 9, (1 << 17) + 1, (1 << bits) - 1], dtype=dt)[:case.arg]
        a, b = np.sort(vals[rng.integers(0, len(vals), na)]), np.sort(vals[rng.integers(0, len(vals), nb)])
    elif case.kind == "high":
        a, b = rand_sorted(na, 1 << 63), rand_sorted(nb, 1 << 63)
    else:
        assert case.kind == "masked"         # ordered by the masked bytes, anything above them
        m = case.mask_bits
        a = rand_sorted(na, 0, min(case.mask, 4000)) | (rng.integers(0, (1 << (bits - m)) - 1, na, dtype=dt, endpoint=True) << dt(m))
        b = rand_sorted(nb, 0, min(case.mask, 4000)) | (rng.integers(0, (1 << (bits - m)) - 1, nb, dtype=dt, endpoint=True) << dt(m))
    top = (1 << 31) - 1 - B_VAL_ADD
    av = rng.integers(0, (1 << 31) - 1, len(a), dtype=np.uint32, endpoint=True)
    bv = rng.integers(0, top, len(b), dtype=np.uint32, endpoint=True)
    if case.kind == "random" and case.arg == 1:
        av[::7] = (1 << 31) - 1; bv[::5] = top               # values of 2^31 - 1 on both sides
    return MergeInput(a.astype(dt), av, b.astype(dt), bv, B_VAL_ADD, runs)


def merge_reference(inp: MergeInput, mask: int):
    """-> (keys, values): the stable merge on key & mask; stability puts a's element first on a tie"""
    dt = inp.a_keys.dtype
    keys = np.concatenate([inp.a_keys, inp.b_keys])
    vals = np.concatenate([inp.a_vals, (inp.b_vals + np.uint32(inp.b_val_add)).astype(np.uint32)])
    order = np.argsort(keys & dt.type(mask), kind="stable")
    return keys[order], vals[order]
