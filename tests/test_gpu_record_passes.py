"""The record-sized passes of the dictionary build under option "lean_records" 1 (the default) and 0.

"lean_records" 1: K-rle runs in kernels of its own (k_rle_tile_sums / k_rle_apply: a wave owns 512 consecutive k-mers, loads
key and gene of each once and takes the neighbours' from the neighbouring lane), the count pass keeps a lane's sixteen records
as bit masks and takes the successors' head bits from the neighbouring lane (gt_count_tile), and the middle launch of a
three-launch scan stages its sums through LDS (k_scan_tile_scan_lds).  0: the generic scan with RecHead / RecScatter, two loads
per record in the count pass, k_scan_tile_scan.  K-rank has one form (its pipelined one was measured and not kept, DESIGN.md
section 4, "Each k-mer and record loaded once"); its edges are here because K-rle reads what it writes.

Every build case, under both values and twice on the same context: the dictionary of pdl_get_dictionary, per-gene and
per-genome lookups, "Total cost" and every genome's Scores block equal the CPU oracle's.  Each set is crafted for a property
(k = 3, at most eight letters) and the property is asserted on the oracle's dictionary alone before the device is asked:
M = k-mers of the stream, U = records, where the runs of one (rank, gene) lie in the sorted stream, where the rank-groups end
among the records.  The K-rank sets also go through an append and a query (k_rank MODE 0).

The tile scan is held against numpy.cumsum through the hook tests/test_gpu_primitives.py uses."""
import functools
import itertools

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

K = 3
LEAN = [1, 0]
T = 2048                                 # k-mers per workgroup of k_rle_tile_sums / k_rle_apply (RLE_TILE), four waves of 512
WAVE_SPAN = 512
ALPHA = H.LETTERS[:8]
SHORT = [np.frombuffer(x, np.uint8) for x in (b"AC", b"DE", b"FG", b"HI")]       # every letter of ALPHA, no k-mer


def _arrays(genes, genomes=3):
    """genes (arrays of letters) -> (residues, offsets, genome_of): genomes of consecutive genes, as equal as they come"""
    n = len(genes)
    g = min(genomes, n)
    gs = H.as_gene_set(genes, np.arange(n) * g // n, [-1] * n)
    return gs.residues, gs.offsets, gs.genome_of


class _Want:
    """What the oracle says about a set; made once per set, never changed."""

    def __init__(self, arrays):
        from oracle import binding as ob
        ora = ob.Oracle(*arrays, K)
        self.arrays, self.genomes = arrays, int(ora.genomes)
        self.dictionary = np.array(ora.dictionary())
        self.total_visited, self.kseq = np.array(ora.total_visited()), np.array(ora.kseq_lengths())
        self.total_cost = int(ora.total_cost)
        self.genome_cost = [int(ora.genome_cost(g)) for g in range(self.genomes)]
        self.scores = [ora.scores(g) for g in range(self.genomes)]
        self.M, self.U = int(ora.kmer_occurrences), len(self.dictionary)
        ora.close()
        assert self.M == int(self.kseq.sum())
        # The oracle's dictionary has the reference's fold in it: a last record that opens a group of its own stands inside the
        # group before it, at its gene's place.  In (rank, gene) order the records are the sorted stream's again.
        d = self.sorted = self.dictionary[np.lexsort((self.dictionary["seq"], self.dictionary["rank"]))]
        # stream position of every record's first and last k-mer (the counts are the run lengths where none is saturated)
        self.pos = np.r_[0, np.cumsum(d["count"].astype(np.int64))][:-1]
        self.run_end = self.pos + d["count"] - 1
        # first and last record of every rank-group as the count pass meets them, behind the fold
        heads = np.flatnonzero(np.r_[True, d["rank"][1:] != d["rank"][:-1]])
        self.folded = bool(self.U >= 2 and heads[-1] == self.U - 1)
        if self.folded:
            heads = heads[:-1]
        self.group_start = heads
        self.group_end = np.r_[heads[1:] - 1, self.U - 1]


def _check_build(nat, w, label):
    ranks, seqs, counts = nat.dictionary()
    d = w.dictionary
    assert nat.cost.kmer_occurrences == w.M and nat.cost.dictionary_records == w.U, label
    assert np.array_equal(ranks, d["rank"]), f"{label}: ranks"
    assert np.array_equal(seqs, d["seq"]), f"{label}: genes"
    assert np.array_equal(counts, d["count"]), f"{label}: counts"
    cost, kl = nat.sequence_costs()
    assert np.array_equal(cost, w.total_visited), f"{label}: per-gene lookups"
    assert np.array_equal(kl, w.kseq), f"{label}: k-mers per gene"
    assert nat.cost.total_cost == w.total_cost, f"{label}: total cost"
    for g in range(w.genomes):
        assert nat.genome_cost(g) == w.genome_cost[g], f"{label}: genome {g} cost"
        H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), w.scores[g], f"{label} genome {g}")


def _build_twice(w, lean, name):
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.open()
    nat.set_option("lean_records", lean)
    for rep in range(2):
        nat.preprocess(K, *w.arrays)
        _check_build(nat, w, f"{name} lean_records={lean} build {rep}")
    nat.close()


# ---- sets --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kmers_in_rank_order():
    """the 512 k-mers over ALPHA as the oracle orders them: one gene per k-mer, its dictionary names the genes in rank order"""
    from oracle import binding as ob
    kmers = [bytes(t) for t in itertools.product(ALPHA.tobytes(), repeat=K)]
    ora = ob.Oracle(*_arrays([np.frombuffer(x, np.uint8) for x in kmers], 2), K)
    order = [kmers[int(i)] for i in np.array(ora.dictionary())["seq"]]
    ora.close()
    assert len(order) == len(kmers)
    return order


def _from_spec(spec, seed):
    """spec[i] = the multiplicities of the i-th k-mer (in rank order) in the genes that hold it: 1 -> a gene that is the k-mer,
    n > 1 -> a gene of n + 2 equal letters (the k-mer is one letter three times).  Genes in random order, the SHORT genes among
    them: every letter of ALPHA occurs, so the ranks are those of _kmers_in_rank_order."""
    order = _kmers_in_rank_order()
    genes = []
    for kmer, mults in zip(order, spec):
        for n in mults:
            if n > 1:
                assert len(set(kmer)) == 1
            genes.append(np.frombuffer(kmer[:1] * (n + 2) if n > 1 else kmer, np.uint8))
    genes += SHORT
    perm = np.random.default_rng(seed).permutation(len(genes))
    return _arrays([genes[i] for i in perm])


def _group_set(sizes, seed=1):
    """rank-groups of the given sizes, in record order; one record per gene (U = M = the sum)"""
    assert len(sizes) <= 512
    return _from_spec([[1] * s for s in sizes] + [[]] * (512 - len(sizes)), seed)


def _sizes_to(u, seed):
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < u:
        sizes.append(min(int(rng.integers(1, 21)), u - sum(sizes)))
    return sizes


def _random_set(m, seed, letters=4, lens=(10, 40)):
    """random genes over a few letters with m k-mers in all (the last gene cut to fit), a gene shorter than k after every
    seventh: many runs of one (rank, gene), large rank-groups"""
    rng = np.random.default_rng(seed)
    genes, left = [], m
    while left > 0:
        take = min(int(rng.integers(lens[0], lens[1] + 1)), left)
        genes.append(ALPHA[rng.integers(0, letters, take + K - 1)])
        left -= take
        if len(genes) % 7 == 0:
            genes.append(ALPHA[rng.integers(0, letters, int(rng.integers(1, K)))])
    return _arrays(genes)


def _run_set():
    """runs of one (rank, gene) at chosen places of the sorted stream: the k-mers of one letter, each in ONE gene"""
    order = _kmers_in_rank_order()
    homo = [i for i, x in enumerate(order) if len(set(x)) == 1]
    assert len(homo) == 8 and homo[0] == 0 and homo[-1] == len(order) - 1
    spec = [[] for _ in order]
    at = 0

    def fill(lo, hi, upto):              # single-k-mer genes over the k-mers order[lo:hi] until the stream holds `upto` k-mers
        nonlocal at
        ks = list(range(lo, hi))
        assert ks and upto >= at
        for j in range(upto - at):
            spec[ks[j % len(ks)]].append(1)
        at = upto

    def run(i, n):
        nonlocal at
        spec[homo[i]].append(n)
        at += n

    run(0, 70)                                               # 0 .. 69: 70 long, from one gene of k + 69 equal letters
    fill(homo[0] + 1, homo[1], WAVE_SPAN - 12); run(1, 30)   # crosses the first wave's end
    fill(homo[1] + 1, homo[2], T - 8); run(2, 20)            # crosses the first tile's end
    fill(homo[2] + 1, homo[7], 2 * T + 100); run(7, 5)       # ends at M - 1
    return _from_spec(spec, 5)


def _span_set():
    """K-rank tiles (4096 stream slots) over more than 128 genes, over 65 .. 128 genes and over fewer, genes shorter than k
    among them"""
    rng = np.random.default_rng(11)
    genes = []
    for _ in range(5000):
        genes.append(ALPHA[rng.integers(0, 8, K + int(rng.integers(0, 3)))])
        if rng.random() < 0.2:
            genes.append(ALPHA[rng.integers(0, 8, int(rng.integers(1, K)))])
    for i in range(300):
        genes.append(ALPHA[rng.integers(0, 8, int(rng.integers(38, 47)))])
        if i % 10 == 5:
            genes.append(ALPHA[rng.integers(0, 8, 2)])
    for _ in range(40):
        genes.append(ALPHA[rng.integers(0, 8, int(rng.integers(200, 400)))])
    return _arrays(genes)


BORDERS = [64, 1024, 4096]                                   # a round of 64 records, a tile of 1024, a workgroup's 4096
ENDS_AT = [64] + [120] * 8 + [127] * 8 + [1041] + [145] * 7  # groups end at 63, 1023 and 4095; the one of 1041 lies in three tiles
ONES_AT = [63, 1, 1] + [200] * 4 + [158] + [1, 1] + [200] * 15 + [70] + [1, 1]      # groups of one at 63 | 64, 1023 | 1024, 4095 | 4096
RLE_M = [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
COUNT_U = [1, 1023, 1024, 1025, 4095, 4096, 4097]
RANK_M = [4096 + 500, 4096 + 1500, 4096 + 2500, 4096 + 3500, 8192]      # the last tile ends in each of its four trips, and full


@functools.lru_cache(maxsize=None)
def _case(name):
    kind, _, arg = name.partition(":")
    if kind == "m":
        return _Want(_random_set(int(arg), 100 + int(arg)))
    if kind == "u":
        return _Want(_group_set(_sizes_to(int(arg), 200 + int(arg)), seed=int(arg)))
    if kind == "runs":
        return _Want(_run_set())
    if kind == "no_repeat":
        return _Want(_group_set(_sizes_to(3000, 7), seed=7))
    if kind == "one_letter":
        return _Want(_arrays([np.full(2 * T + 5 + K - 1, ALPHA[0], np.uint8)]))
    if kind == "ends_at":                                    # :fold -> the last record opens a group of its own, which is folded
        return _Want(_group_set(ENDS_AT + ([3, 1] if arg == "fold" else [3, 2]), seed=3))
    if kind == "ones_at":
        return _Want(_group_set(ONES_AT + [4, 2], seed=4))
    if kind == "spans":
        return _Want(_span_set())
    raise KeyError(name)


# ---- K-rle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lean", LEAN)
@pytest.mark.parametrize("m", RLE_M)
def test_rle_stream_lengths(m, lean):
    w = _case(f"m:{m}")
    assert w.M == m
    _build_twice(w, lean, f"m:{m}")


@pytest.mark.parametrize("lean", LEAN)
def test_rle_runs_across_wave_and_tile_ends(lean):
    w = _case("runs")
    runs = np.flatnonzero(w.sorted["count"] >= 2)
    first, last, length = w.pos[runs], w.run_end[runs], w.sorted["count"][runs]
    assert w.M > 2 * T and int(w.dictionary["count"].max()) < 1023
    assert ((first < WAVE_SPAN) & (last >= WAVE_SPAN)).any(), "a run across the end of a wave's 512 k-mers"
    assert ((first < T) & (last >= T)).any(), "a run across the end of a tile"
    assert (length == 70).any() and ((first < 64) & (last >= 64) & (length == 70)).any(), "a run of 70"
    assert int(last.max()) == w.M - 1, "a run that ends the stream"
    _build_twice(w, lean, "runs")


@pytest.mark.parametrize("lean", LEAN)
def test_rle_no_repeat_at_all(lean):
    w = _case("no_repeat")
    assert w.U == w.M == 3000 and (w.dictionary["count"] == 1).all()
    _build_twice(w, lean, "no_repeat")


@pytest.mark.parametrize("lean", LEAN)
def test_rle_every_kmer_repeats_its_predecessor(lean):
    w = _case("one_letter")
    assert w.U == 1 and w.M == 2 * T + 5 and len(w.kseq) == 1
    _build_twice(w, lean, "one_letter")


# ---- count pass ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lean", LEAN)
@pytest.mark.parametrize("u", COUNT_U)
def test_count_record_counts(u, lean):
    w = _case(f"u:{u}")
    assert w.U == u == w.M
    _build_twice(w, lean, f"u:{u}")


@pytest.mark.parametrize("lean", LEAN)
@pytest.mark.parametrize("fold", ["fold", "no_fold"])
def test_count_groups_end_on_round_tile_and_block_ends(fold, lean):
    w = _case(f"ends_at:{fold}")
    assert w.folded == (fold == "fold")
    for b in BORDERS:
        assert b - 1 in w.group_end and b in w.group_start, b
    assert w.group_end[-1] == w.U - 1 and w.group_start[-1] == w.U - (4 if w.folded else 2)
    size = w.group_end - w.group_start + 1
    big = int(np.argmax(size))
    assert w.group_end[big] // 1024 - w.group_start[big] // 1024 == 2, "one group in three tiles"
    _build_twice(w, lean, f"ends_at:{fold}")


@pytest.mark.parametrize("lean", LEAN)
def test_count_groups_of_one_on_either_side_of_the_ends(lean):
    w = _case("ones_at")
    for b in BORDERS:
        for u in (b - 1, b):
            assert u in w.group_start and u in w.group_end, (b, u)
    assert not w.folded
    _build_twice(w, lean, "ones_at")


# ---- K-rank --------------------------------------------------------------------------------------------------------------------
def _append_and_query(w, lean, name):
    """the last genome comes as a query and then joins by an append (k_rank MODE 0, K-rle over the new genes' k-mers)"""
    from pandelos_amd.pangene_native import PangeneNative
    res, off, gen = w.arrays
    g_last = w.genomes - 1
    n0 = int(np.searchsorted(gen, g_last))
    r0 = int(off[n0])
    base = (res[:r0], off[:n0 + 1], gen[:n0])
    new = (res[r0:], off[n0:] - off[n0])
    nat = PangeneNative.open()
    nat.set_option("lean_records", lean)
    nat.preprocess(K, *base)
    label = f"{name} lean_records={lean}"
    H.assert_scores_equal(nat.query_scores(*new).as_dict(), w.scores[g_last], f"{label}: query")
    nat.append(*new)
    _check_build(nat, w, f"{label}: append")
    nat.close()


@pytest.mark.parametrize("lean", LEAN)
@pytest.mark.parametrize("m", RANK_M)
def test_rank_last_tile_ends_in_each_trip(m, lean):
    w = _case(f"m:{m}")
    assert w.M == m and w.genomes == 3
    _build_twice(w, lean, f"m:{m}")
    _append_and_query(w, lean, f"m:{m}")


@pytest.mark.parametrize("lean", LEAN)
def test_rank_tiles_over_many_genes(lean):
    w = _case("spans")
    koff = np.r_[0, np.cumsum(w.kseq.astype(np.int64))]
    spans = []                                               # (genes k_rank brackets under a tile, a gene shorter than k between genes that have k-mers)
    for q0 in range(0, w.M, 4096):
        lo = int(np.searchsorted(koff, q0, "right")) - 1
        hi = int(np.searchsorted(koff, min(q0 + 4096, w.M) - 1, "right")) - 1
        inside = w.kseq[lo + 1:hi]
        spans.append((hi - lo + 1, bool((inside == 0).any() and (inside > 0).any())))
    assert any(s > 128 and short for s, short in spans), spans
    assert any(64 < s <= 128 and short for s, short in spans), spans
    assert any(s <= 64 for s, _ in spans), spans
    _build_twice(w, lean, "spans")
    _append_and_query(w, lean, "spans")


# ---- tile scan -------------------------------------------------------------------------------------------------------------------
SCAN_TILE = 2048
TILE_COUNTS = [1, 2, 1023, 1024, 1025, 16383, 16384, 16385]


@functools.lru_cache(maxsize=None)
def _scan_case(tiles):
    n = tiles * SCAN_TILE - 5                                # the last tile is not full
    flags = np.random.default_rng(tiles).integers(0, 4, n, dtype=np.uint32)
    incl = np.cumsum(flags, dtype=np.uint64)
    assert int(incl[-1]) < 2 ** 32
    prefix = (incl - flags).astype(np.uint32)
    flags.setflags(write=False), prefix.setflags(write=False)
    return flags, prefix, int(incl[-1])


@pytest.mark.parametrize("lean", LEAN)
@pytest.mark.parametrize("tiles", TILE_COUNTS)
def test_tile_scan_against_cumsum(tiles, lean):
    import torch
    from pandelos_amd.pangene_native import PangeneNative
    flags, want, want_total = _scan_case(tiles)
    n = len(flags)
    nat = PangeneNative.open()
    nat.set_option("onepass_scan", 0)
    nat.set_option("lean_records", lean)
    d_flags = torch.from_numpy(flags.view(np.int32).copy()).cuda()             # (a writable copy: the cached array is not)
    for rep in range(2):
        d_prefix = torch.full((n + 64,), -1, dtype=torch.int32, device="cuda")
        d_seen = torch.full((n + 64,), -1, dtype=torch.int32, device="cuda")
        d_total = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        nat._check(nat._lib.pdl_test_scan(nat._ctx, d_flags.data_ptr(), n, None, d_prefix.data_ptr(), d_seen.data_ptr(), 0,
                                          d_total.data_ptr(), None))
        label = f"{tiles} tiles lean_records={lean} run {rep}"
        total = d_total.cpu().numpy()
        assert int(total[0]) == want_total and int(total[1]) == -1, label
        got = d_prefix.cpu().numpy().view(np.uint32)
        bad = np.flatnonzero(got[:n] != want)
        assert len(bad) == 0, f"{label}: {len(bad)} prefixes differ, first at {int(bad[0])} (tile {int(bad[0]) // SCAN_TILE})"
        assert (got[n:] == 0xffffffff).all(), f"{label}: written behind the count"
        assert np.array_equal(d_seen.cpu().numpy().view(np.uint32)[:n], flags), f"{label}: flags seen"
    nat.close()
