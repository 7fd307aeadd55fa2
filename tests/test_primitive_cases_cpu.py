"""The case tables of tests/primitive_cases.py, without a device: every case is what its name says — its tile count lies on the
side of the regime constant it is there for, its totals fit 32 bits, its inputs keep the primitive's contract — and the numpy
references agree with a second, naive formulation (a Python loop, `sorted` with a key, a two-pointer merge) on small inputs, so
that they are not held against the code under test only."""
import numpy as np
import pytest

from tests import primitive_cases as P


def _scan_tiles(n):
    return P.tiles_of(n, P.SCAN_TILE)


def test_the_regime_constants_are_the_kernels():
    """read from the sources: a constant that moves there has to move in the table (and the cases with it)"""
    import re
    from pathlib import Path
    src = Path(__file__).resolve().parents[1] / "pandelos_amd" / "csrc"
    scan, sort_h, sort, merge = ((src / f).read_text() for f in ("pdl_scan.h", "pdl_sort.h", "pdl_sort.hip", "pdl_append.h"))

    def const(text, name):
        return re.search(r"constexpr \w+ (?:\w+ = [^,;]+, )*" + name + r" = ([^,;]+)[,;]", text).group(1).strip()

    assert (const(scan, "SCAN_THREADS"), const(scan, "SCAN_ITEMS")) == ("256", "8") and P.SCAN_TILE == 256 * 8
    assert int(const(scan, "SCAN_INLINE_TILES")) == P.SCAN_INLINE_TILES
    assert 1024 * int(const(scan, "TS_ITEMS")) == P.SCAN_ONE_TRIP_TILES and "base += 1024" in scan and P.SCAN_CARRY_TRIP == 1024
    assert const(scan, "LB_CHUNK") == "PDL_WAVE" and P.LB_CHUNK == 64
    assert int(const(sort_h, "PDL_RADIX_TILE")) == P.RADIX_TILE and int(const(sort_h, "PDL_RADIX_BINS")) == P.RADIX_BINS
    assert (const(sort, "RO_THREADS"), const(sort, "RO_ITEMS")) == ("1024", "4") and P.RADIX_TILE == 1024 * 4       # RO_TRIP
    assert int(const(sort, "RO_MAX_TILES")) == P.RO_MAX_TILES
    assert (const(merge, "MG_THREADS"), const(merge, "MG_ITEMS")) == ("256", "8") and P.MG_ITEMS == 8 and P.SCAN_TILE == 256 * 8


def test_scan_sizes_fall_on_both_sides_of_every_switch():
    tiles = [_scan_tiles(n) for n in P.SCAN_N]
    assert tiles[:7] == [1, 1, 1, 1, 1, 1, 2]
    assert tiles[7:11] == [P.SCAN_INLINE_TILES, P.SCAN_INLINE_TILES + 1, P.SCAN_ONE_TRIP_TILES, P.SCAN_ONE_TRIP_TILES + 1]
    assert P.SCAN_N[7] % P.SCAN_TILE == 0 and P.SCAN_N[9] % P.SCAN_TILE == 0            # the last tile before the switch is full
    carry = tiles[11]
    assert carry > P.SCAN_ONE_TRIP_TILES and carry // P.SCAN_CARRY_TRIP >= 18 and carry % P.SCAN_CARRY_TRIP == 5       # 18 full trips, a ragged one
    assert P.SCAN_N[11] % P.SCAN_TILE == P.SCAN_TILE - 3
    assert {c.n_bound for c in P.SCAN_SIZE_CASES} == set(P.SCAN_N) and {c.kind for c in P.SCAN_SIZE_CASES} == {"bits", "small"}
    below, above = (_scan_tiles(c.n_bound) for c in P.SCAN_COUNT_CASES[::5])
    assert below == 5 and above == 1030 and below <= P.SCAN_INLINE_TILES < above
    for t in P.SCAN_BOUND_TILES:
        counts = sorted(c.d_n for c in P.SCAN_COUNT_CASES if _scan_tiles(c.n_bound) == t)
        bound = t * P.SCAN_TILE - 9
        assert counts == [0, 1, P.SCAN_TILE, bound - 1, bound]
    assert _scan_tiles(P.SCAN_EDGE_CASES[3].n_bound) > P.SCAN_INLINE_TILES >= _scan_tiles(P.SCAN_EDGE_CASES[2].n_bound)


def test_onepass_sizes_fall_on_both_sides_of_the_chunk_levels():
    assert [_scan_tiles(c.n_bound) for c in P.ONEPASS_CASES] == list(P.ONEPASS_TILES)
    chunk, level2 = P.LB_CHUNK, P.LB_CHUNK * P.LB_CHUNK                                # 64 tiles a chunk, 64 chunks a look-back step
    assert {chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, level2, level2 + 1} <= set(P.ONEPASS_TILES)
    assert max(P.ONEPASS_TILES) > P.SCAN_ONE_TRIP_TILES
    assert [_scan_tiles(c.n_bound) for c in P.ONEPASS_SEQUENCE] == [4097, 65, 16385, 1, 4097]
    c = P.ONEPASS_COUNT_CASES[0]
    assert _scan_tiles(c.count) == chunk + 1 < _scan_tiles(c.n_bound)


@pytest.mark.parametrize("case", P.ALL_SCAN_CASES, ids=lambda c: c.name)
def test_scan_totals_fit_32_bits(case):
    flags = P.scan_flags(case)
    assert flags.dtype == np.uint32 and len(flags) == case.n_bound
    assert int(flags.max(initial=0)) <= 1023
    prefix, total = P.scan_reference(flags, case.count)
    assert total < 1 << 32 and len(prefix) == case.count
    assert total == int(flags[:case.count].sum(dtype=np.uint64))
    if case.kind == "bits":
        assert 0 < total < case.count or case.count < 64
    if case.kind == "small" and case.count > 4096:
        assert total > case.count // 8 or case.n_bound > 1 << 22
        assert total > 1 << 20


def test_scan_near_wrap_total():
    flags = P.scan_flags(P.SCAN_NEAR_WRAP)
    _, total = P.scan_reference(flags, P.SCAN_NEAR_WRAP.count)
    assert total == 4290778107 and (1 << 32) - total < 1 << 22


def test_scan_reference_against_a_loop():
    for case in (P.ScanCase("loop_small", 5000, "small", seed=9), P.ScanCase("loop_bits", 4097, "bits", seed=8),
                 P.ScanCase("loop_count", 5000, "small", d_n=2049, seed=7), P.ScanCase("loop_none", 300, "small", d_n=0, seed=6)):
        flags = P.scan_flags(case)
        prefix, total = P.scan_reference(flags, case.count)
        run, want = 0, []
        for f in flags[:case.count].tolist():
            want.append(run); run += f
        assert prefix.tolist() == want and total == run


@pytest.mark.parametrize("case", P.OFFSETS_CASES, ids=lambda c: c.name)
def test_offsets_tables_keep_the_contract(case):
    counts = P.offsets_counts(case)
    t = case.n_tiles
    assert counts.shape == (P.RADIX_BINS, t) and counts.dtype == np.uint32
    per_tile = counts.sum(axis=0, dtype=np.uint64)
    assert int(per_tile.max()) <= P.RADIX_TILE                                         # a tile has 4096 elements
    assert int(per_tile.sum()) <= t * P.RADIX_TILE and int(per_tile.sum()) < 1 << 32
    assert int(per_tile[0]) == P.RADIX_TILE and int(counts[:, 0].max()) == P.RADIX_TILE   # a tile of one digit
    if case.zero_suffix:
        assert not counts[:, t - case.zero_suffix:].any() and counts[:, t - case.zero_suffix - 1].any()
    else:
        assert t <= 2
    lean_offs, digit_total = P.offsets_reference(counts, True)
    offs, total = P.offsets_reference(counts, False)
    assert int(digit_total.sum(dtype=np.uint64)) == total == int(per_tile.sum())
    base = np.cumsum(digit_total, dtype=np.uint64) - digit_total                       # what the scatter adds to the lean form
    assert np.array_equal(lean_offs + base[:, None].astype(np.uint32), offs)


def test_offsets_sizes_fall_on_both_sides_of_every_switch():
    t = P.OFFSETS_TILES
    trip = P.RADIX_TILE
    assert t == (1, 2, trip - 1, trip, trip + 1, 2 * trip, 2 * trip + 1, P.RO_MAX_TILES, P.RO_MAX_TILES + 1)
    assert [P.tiles_of(x, trip) for x in t] == [1, 1, 1, 1, 2, 2, 3, 16, 17]           # trips of k_rs_offsets over a row
    for lean in (0, 1):
        for onepass in (0, 1):
            took = [x for x in t if P.offsets_lean_expected(x, lean, onepass)]
            assert took == ([x for x in t if x <= P.RO_MAX_TILES] if lean and not onepass else [])
    # the three-launch scan over the table: on both sides of its own switches too
    scan_tiles = [_scan_tiles(P.RADIX_BINS * x) for x in t]
    assert min(scan_tiles) == 1 and any(x <= P.SCAN_INLINE_TILES for x in scan_tiles) and max(scan_tiles) <= P.SCAN_ONE_TRIP_TILES


def test_offsets_reference_against_a_loop():
    counts = P.offsets_counts(P.OffsetsCase("loop", 9, 3))
    lean_offs, digit_total = P.offsets_reference(counts, True)
    offs, total = P.offsets_reference(counts, False)
    run = 0
    for d in range(P.RADIX_BINS):
        row = 0
        for t in range(9):
            assert int(offs[d, t]) == run and int(lean_offs[d, t]) == row
            run += int(counts[d, t]); row += int(counts[d, t])
        assert int(digit_total[d]) == row
    assert total == run


ALL_SORT = P.all_sort_cases()


def test_sort_table_holds_every_listed_case():
    names = [c.name for c in ALL_SORT]
    assert len(set(names)) == len(names)
    for kb, vb in P.WIDTHS:
        mine = [c for c in ALL_SORT if (c.key_bytes, c.val_bytes) == (kb, vb)]
        assert {c.n for c in P.sort_size_cases(kb, vb)} == {1, 63, 64, 65, 1023, 1025, 4095, 4096, 4097, 8193, 100003}
        ends = {(c.end_bit, c.below) for c in P.sort_end_bit_cases(kb, vb)}
        want = set(range(1, 17)) | {17, 24, 31, 32} | ({33, 40, 63, 64} if kb == 8 else set())
        assert {(e, b) for e in want for b in (True, False)} <= ends
        assert {c.begin_bit for c in P.sort_begin_bit_cases(kb, vb)} == {0, 8, 24} and all(c.end_bit == 32 for c in P.sort_begin_bit_cases(kb, vb))
        assert {c.pattern for c in mine} >= set(P.SORT_PATTERNS) | ({"high"} if kb == 8 else set())
        assert any(c.iota for c in mine) and any(not c.iota for c in mine)
        for t in P.SORT_BOUND_TILES:
            n = t * P.RADIX_TILE - 5
            assert P.tiles_of(n, P.RADIX_TILE) == t
            assert sorted(c.d_n for c in P.sort_count_cases(kb, vb) if c.n == n) == [0, 1, P.RADIX_TILE, n - 1, n]
            assert len([c for c in P.sort_filed_cases(kb, vb) if c.n == n]) == 2
        big = [P.tiles_of(c.n, P.RADIX_TILE) for c in P.sort_big_cases(kb, vb)]
        assert big == [P.RADIX_TILE, P.RADIX_TILE + 1, 2 * P.RADIX_TILE + 1]              # one, two and three trips of k_rs_offsets
        assert all(c.end_bit <= 16 and t <= P.RO_MAX_TILES for c, t in zip(P.sort_big_cases(kb, vb), big))
        # ... and the three-launch scan of their tables (lean_radix 0) on both sides of SCAN_INLINE_TILES
        assert [_scan_tiles(P.RADIX_BINS * t) <= P.SCAN_INLINE_TILES for t in big] == [True, True, False]


@pytest.mark.parametrize("case", ALL_SORT, ids=lambda c: c.name)
def test_sort_keys_are_what_the_case_says(case):
    keys = P.sort_keys(case)
    assert len(keys) == case.n and keys.dtype == (np.uint64 if case.key_bytes == 8 else np.uint32)
    top = P.sort_top(case)
    end = min(max(case.end_bit, 1), case.key_bits)
    assert case.begin_bit % 8 == 0 and case.begin_bit < top <= case.key_bits
    if case.below:
        assert top == end and int(keys.max()) < 1 << end
    else:
        assert top % 8 == 0 and top - end < 8
        if case.pattern == "random" and top < case.key_bits and case.n > 1000:
            assert int(keys.max()) >= 1 << top                                          # bits above what the sort looks at
    if case.pattern == "random" and case.n > 1000 and case.begin_bit:
        assert len(np.unique(keys & keys.dtype.type((1 << case.begin_bit) - 1))) > 100      # the lower bits are random
        low = keys & keys.dtype.type((1 << case.begin_bit) - 1)
        assert (np.diff(low.astype(np.int64)) < 0).any()                                # and not in the order earlier passes would leave
    if case.pattern == "equal":
        assert len(np.unique(keys)) == 1
    if case.pattern == "descending":
        assert (keys[1:] < keys[:-1]).all() and len(np.unique(keys)) == case.n
    if case.pattern == "one_differs":
        odd = np.flatnonzero(keys != keys[0])
        assert len(odd) == 1 and bin(int(keys[odd[0]]) ^ int(keys[0])).count("1") == 1
    if case.pattern == "tile_digit":
        low = (keys & keys.dtype.type(0xFF)).reshape(-1)[:case.n // P.RADIX_TILE * P.RADIX_TILE].reshape(-1, P.RADIX_TILE)
        assert (low == low[:, :1]).all() and len(np.unique(low[:, 0])) == len(low)
    if case.pattern == "round_distinct":
        for shift in (0, 8):
            d = ((keys >> keys.dtype.type(shift)) & keys.dtype.type(0xFF)).astype(np.int64)
            win = np.lib.stride_tricks.sliding_window_view(d, 64)
            assert (np.sort(win, axis=1)[:, 1:] != np.sort(win, axis=1)[:, :-1]).all()
    if case.pattern == "high":
        assert int(keys.min()) >= 1 << 63
    if case.val_bytes == 8 and not case.iota and case.n < P.SORT_BIG_N[0]:
        assert int(P.sort_values(case).min()) >= 1 << 32
    if case.filed:
        counts = P.sort_first_counts(case, keys)
        t = P.tiles_of(case.n, P.RADIX_TILE)
        assert counts.shape == (P.RADIX_BINS, t) and int(counts.sum()) == case.count
        live = P.tiles_of(case.count, P.RADIX_TILE)
        assert not counts[:, live:].any() and int(counts.sum(axis=0).max()) <= P.RADIX_TILE


def test_sort_reference_against_sorted_with_a_key():
    cases = (P.SortCase("s1", 4, 4, 3000, 12), P.SortCase("s2", 4, 4, 3000, 12, below=True, seed=1), P.SortCase("s3", 8, 4, 3000, 40, seed=2),
             P.SortCase("s4", 4, 8, 3000, 32, begin_bit=24, seed=3), P.SortCase("s5", 8, 4, 3000, 32, begin_bit=8, seed=4),
             P.SortCase("s6", 4, 4, 3000, 0, below=True, seed=5), P.SortCase("s7", 4, 4, 3000, 40, seed=6),
             P.SortCase("s8", 4, 4, 3000, 16, d_n=1234, seed=7), P.SortCase("s9", 8, 4, 3000, 64, pattern="high", seed=8))
    for case in cases:
        keys, vals = P.sort_keys(case), P.sort_values(case)
        end = min(max(case.end_bit, 1), case.key_bits)
        top = end if case.below else min(-(-end // 8) * 8, case.key_bits)
        field = lambda k: (k >> case.begin_bit) % (1 << (top - case.begin_bit))
        order = sorted(range(case.count), key=lambda i: field(int(keys[i])))            # (sorted is stable)
        got_k, got_v = P.sort_reference(case, keys, vals)
        assert got_k.tolist() == [int(keys[i]) for i in order] and got_v.tolist() == [int(vals[i]) for i in order], case.name
        got_k, got_v = P.sort_reference(case, keys, None)
        assert got_v.tolist() == order and got_v.dtype == (np.uint64 if case.val_bytes == 8 else np.uint32), case.name


ALL_MERGE = P.all_merge_cases()


def test_merge_table_holds_every_listed_case():
    names = [c.name for c in ALL_MERGE]
    assert len(set(names)) == len(names)
    for kb in (4, 8):
        mine = [c for c in ALL_MERGE if c.key_bytes == kb]
        assert any(c.na == 0 and c.nb for c in mine) and {c.na % 4 for c in mine if c.nb == 0 and c.na > 4} == {1, 2, 3}
        assert {c.na + c.nb for c in mine} >= set(P.MERGE_TOTALS)
        assert {c.kind for c in mine} >= {"equal", "b_below", "b_above", "one_b_per_tile", "tie_runs", "few", "masked"}
    assert sorted(c.mask_bits for c in ALL_MERGE if c.kind == "masked" and c.key_bytes == 8) == [8, 16, 24, 32, 40, 48, 56]
    assert [c.mask_bits for c in ALL_MERGE if c.kind == "masked" and c.key_bytes == 4] == [16]
    assert any(c.na + c.nb == 5_000_000 for c in ALL_MERGE)


@pytest.mark.parametrize("case", ALL_MERGE, ids=lambda c: c.name)
def test_merge_inputs_are_what_the_case_says(case):
    inp = P.merge_input(case)
    dt = np.uint64 if case.key_bytes == 8 else np.uint32
    na, nb = len(inp.a_keys), len(inp.b_keys)
    if case.kind != "tie_runs":
        assert (na, nb) == (case.na, case.nb)
    assert na + nb < 1 << 32 and inp.a_keys.dtype == dt and inp.b_keys.dtype == dt
    mask = dt(case.mask)
    for k in (inp.a_keys, inp.b_keys):
        m = k & mask
        assert (m[1:] >= m[:-1]).all()                                                  # sorted on key & mask
    assert inp.b_val_add and int(inp.a_vals.max(initial=0)) <= (1 << 31) - 1
    assert int(inp.b_vals.astype(np.uint64).max(initial=0)) + inp.b_val_add <= (1 << 31) - 1
    keys, vals = P.merge_reference(inp, case.mask)
    if case.kind == "equal":
        assert len(np.unique(np.concatenate([inp.a_keys, inp.b_keys]))) == 1 and na > 2 * P.SCAN_TILE and nb > 2 * P.SCAN_TILE - 1
        assert np.array_equal(vals[:na], inp.a_vals)                                    # a first, whole
    if case.kind == "b_below":
        assert int(inp.b_keys.max()) < int(inp.a_keys.min())
    if case.kind == "b_above":
        assert int(inp.b_keys.min()) > int(inp.a_keys.max())
    if case.kind == "one_b_per_tile":
        from_b = np.flatnonzero(np.isin(keys, inp.b_keys))
        assert from_b.tolist() == [t * P.SCAN_TILE + case.arg for t in range(nb)] and P.tiles_of(na + nb, P.SCAN_TILE) == nb + 1
    if case.kind == "few":
        assert len(np.unique(keys)) == case.arg == 4 and na + nb == 50000
    if case.kind == "high":
        assert int(keys.min()) >= 1 << 63
    if case.kind == "masked":
        above = np.concatenate([inp.a_keys, inp.b_keys]) >> dt(case.mask_bits)
        assert len(np.unique(above)) > 100 or case.mask_bits >= 56                      # the upper bytes are random ...
        m = keys & mask
        ties = np.flatnonzero(m[1:] == m[:-1])
        assert len(ties) > 100 and (keys[ties + 1] != keys[ties]).any()                 # ... and differ inside the ties
    if case.kind == "random" and case.arg == 1:
        assert int(vals.max()) == (1 << 31) - 1 and int(inp.a_vals.max()) == (1 << 31) - 1
    if case.kind == "tie_runs":
        lengths = set()
        assert len(inp.tie_runs) == len(P.TIE_SHORT) + 3
        for lo, hi in inp.tie_runs:
            run = keys[lo:hi]
            assert (run == run[0]).all() and (lo == 0 or keys[lo - 1] != run[0]) and keys[hi] != run[0]
            la = int((inp.a_keys == run[0]).sum())
            lengths |= {la, hi - lo - la}
            assert np.array_equal(vals[lo:lo + la], inp.a_vals[inp.a_keys == run[0]])   # a's elements first
            boundary = -(-lo // P.SCAN_TILE) * P.SCAN_TILE
            assert lo < boundary < hi                                                   # crosses a tile diagonal ...
            assert lo < lo + la < hi and (lo + la) % P.MG_ITEMS != 0                    # a meets b between two diagonals
            assert any(x % P.MG_ITEMS == 0 for x in range(lo + 1, hi))
        assert lengths == set(P.TIE_SHORT) | set(P.TIE_LONG)


def test_merge_reference_against_two_pointers():
    for case in (P.MergeCase("m1", 4, "random", 700, 500, seed=1), P.MergeCase("m2", 8, "masked", 900, 800, mask_bits=8, seed=2),
                 P.MergeCase("m3", 4, "few", 600, 900, arg=4, seed=3), P.MergeCase("m4", 4, "equal", 50, 70), P.MergeCase("m5", 8, "random", 0, 40, seed=4)):
        inp = P.merge_input(case)
        a, b, mask = inp.a_keys.tolist(), inp.b_keys.tolist(), case.mask
        i = j = 0
        want_k, want_v = [], []
        while i < len(a) or j < len(b):
            if j >= len(b) or (i < len(a) and (a[i] & mask) <= (b[j] & mask)):
                want_k.append(a[i]); want_v.append(int(inp.a_vals[i])); i += 1
            else:
                want_k.append(b[j]); want_v.append(int(inp.b_vals[j]) + inp.b_val_add); j += 1
        keys, vals = P.merge_reference(inp, mask)
        assert keys.tolist() == want_k and vals.tolist() == want_v, case.name
