"""Every entry point under every non-default form of the shared stages (pdl_set_option), and the switch of a form on a built
context: the forms, the scenarios and the shapes of tests/test_gpu_option_forms.py, in one place.

A scenario runs one entry point on the device under the given options and compares it, byte for byte (H.raw), with the CPU
reference the entry point's own test file compares it with; the references (Reference, lru_cache) are made once per process on the
CPU and never come from a device run.  tests/test_option_forms_cpu.py proves, without a device, that the sets lie beyond the tile
and chunk constants the forms differ in.  pdl_split_first_level and pdl_pan_curves call neither a scan nor a sort: left out."""
from __future__ import annotations

import json
from functools import lru_cache

import numpy as np

from tests import helpers as H

# ---- the forms -------------------------------------------------------------------------------------------------------------------
DEFAULTS = {"onepass_scan": 0, "lean_radix": 1, "lean_records": 1, "fused_glue": 1, "order_subwave": 1, "order_wide_merged": 1,
            "order_offsets": 2, "sift_threshold": 1, "host_mirror": 1, "stage_timers": 1}
FORMS = {
    "onepass_scan": (("onepass_scan", 1),),              # every scan in one launch; K-rle and the radix passes in their former forms with it
    "full_radix": (("lean_radix", 0),),                  # k_rs_hist + a scan of the count table per pass
    "former_records": (("lean_records", 0),),            # RecHead / RecScatter, the former count body, k_scan_tile_scan
    "glue_apart": (("fused_glue", 0),),
    "klen_one_launch": (("fused_glue", 65536),),
    "order_wave_per_row": (("order_subwave", 0),),
    "order_32_lanes": (("order_subwave", 32),),
    "order_wide_apart": (("order_wide_merged", 0),),
    "order_two_scans": (("order_offsets", 0),),
    "sift_seen_twice": (("sift_threshold", 0),),
    "no_host_mirror": (("host_mirror", 0),),
    "no_stage_timers": (("stage_timers", 0),),           # (the stages then report no times: the re-key helpers compare the total only)
    "all_former": (("lean_radix", 0), ("lean_records", 0), ("fused_glue", 0), ("order_subwave", 0), ("order_offsets", 0), ("sift_threshold", 0)),
}
# the forms of stages that run again over what a build left (test_form_switched_on_a_built_context), and the calls that do so
LATE_FORMS = ("onepass_scan", "full_radix", "former_records", "glue_apart", "klen_one_launch", "all_former")
LATE_SCENARIOS = ("append", "remove", "rekey", "batches", "query")
DIRECTIONS = ("to", "from")

# ---- the regimes: kernel constants and what the sets must pass -----------------------------------------------------------------------
SCAN_TILE = 2048                      # pdl_scan.h: elements of one workgroup of a scan (SCAN_THREADS * SCAN_ITEMS)
LB_CHUNK = 64                         # pdl_scan.h: tiles of one look-back chunk of k_scan_onepass (PDL_WAVE)
SCAN_INLINE_TILES = 1024              # pdl_scan.h: up to so many tiles a three-launch scan has no middle launch
RS_TILE = 4096                        # pdl_sort.hip: keys of one workgroup of a radix pass (RS_THREADS * RS_ROUNDS)
RLE_TILE = 2048                       # pdl_dict.hip: k-mers of one workgroup of K-rle (RLE_WAVES * RLE_SPAN)
MIN_GENES = SCAN_TILE                 # N above it: K-len's scan has more than one tile
MIN_KMERS = LB_CHUNK * SCAN_TILE      # M above it: the look-back crosses a chunk, K-rle has more than 64 tiles, a sort more than 32
MIN_CELLS = SCAN_TILE                 # emitted cells of a context above it
MIN_EDGES = SCAN_TILE                 # best-hit edges of a context above it: both edge compactions leave one tile
MIN_QUERY_GENES = SCAN_TILE           # genes of the big held-out genome above it: RowCntFlag / FinOffApply and K-place's scans leave one tile
MIN_LARGE_KMERS = SCAN_INLINE_TILES * SCAN_TILE       # k-mers above it: a three-launch scan has its middle launch

FULL_SHAPE = dict(genomes=12, genes_per_genome=300, mean_len=70, sub_rate=0.1, seed=1616)
MID_GENOMES = 9                       # the mid-size set: the first nine genomes; 9, 10 and 11 are the held-out ones
MIDDLE = 4                            # the genome "remove" takes from the middle
BIG_QUERY_GENES, BIG_QUERY_LEN = 2250, 40
PROFILE_GENES, PROFILE_GENOMES, PROFILE_SEED = 140_000, 24, 5
PROFILE_SLAB_BYTES = PROFILE_GENOMES * 8 * 3          # three words of every genome per slab of pdl_genome_matrix
LARGE = "mycoplasma64_standin"        # 17 M k-mers: the only set above MIN_LARGE_KMERS
LARGE_FORMS = ("onepass_scan", "full_radix", "former_records", "all_former")


def in_force(options, late=()):
    """the options a context ends with: `options` before its build, `late` behind it"""
    return tuple(options) + tuple(late)


# ---- the sets (numpy only) ----------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def full():
    from pandelos_amd.synth import make_gene_set
    return make_gene_set(**FULL_SHAPE)


@lru_cache(maxsize=None)
def mid_k() -> int:
    from pandelos_amd.calculate_k import calculate_k
    return calculate_k(arrays("mid")[0])


def _genomes(lo, hi):
    """(residues, offsets from 0, genome ids from 0) of genomes lo..hi-1 of full(), whose genomes lie one after the other"""
    gs = full()
    ids = np.flatnonzero((gs.genome_of >= lo) & (gs.genome_of < hi))
    a, b = int(ids[0]), int(ids[-1]) + 1
    assert b - a == len(ids)
    off = gs.offsets[a:b + 1].astype(np.uint64)
    return gs.residues[int(off[0]):int(off[-1])].copy(), off - off[0], (gs.genome_of[a:b] - lo).astype(np.uint32)


@lru_cache(maxsize=None)
def held_out(j: int):
    """(residues, offsets) of genome j of full() as a query"""
    return _genomes(j, j + 1)[:2]


def _pack(genes):
    off = np.zeros(len(genes) + 1, np.uint64)
    np.cumsum([len(g) for g in genes], out=off[1:])
    return np.concatenate(genes).astype(np.uint8), off


@lru_cache(maxsize=None)
def big_query():
    """BIG_QUERY_GENES genes of about BIG_QUERY_LEN residues: the heads of the mid-size set's genes with a few substitutions"""
    res, off, _ = arrays("mid")
    rng = np.random.default_rng(77)
    off = off.astype(np.int64)
    genes = []
    for i in range(BIG_QUERY_GENES):
        g = res[off[i]:off[i] + int(rng.integers(BIG_QUERY_LEN - 4, BIG_QUERY_LEN + 5))].copy()       # (cut at the gene's end or inside the next: both fine)
        m = rng.random(len(g)) < 0.05
        g[m] = H.LETTERS[rng.integers(0, 20, int(m.sum()))]
        genes.append(g)
    return _pack(genes)


@lru_cache(maxsize=None)
def new_letter_query():
    """genome 10 with an X in about one residue of nine: a letter the base lacks (option "query_rekey")"""
    from tests.test_rekey_cpu import with_letters
    res, off = held_out(10)
    off = off.astype(np.int64)
    return _pack([np.frombuffer(with_letters(res[off[i]:off[i + 1]].tobytes(), b"X", 900 + i), np.uint8) for i in range(len(off) - 1)])


QUERIES = {"9": lambda: held_out(9), "10": lambda: held_out(10), "11": lambda: held_out(11), "big": big_query, "x": new_letter_query}


@lru_cache(maxsize=None)
def arrays(name: str):
    """"mid", "mid-last" (its first eight genomes), "mid-two" (seven), "mid-middle" (without genome MIDDLE), "mid+<query>" -> (residues, offsets, genome ids)"""
    from pandelos_amd.remove import remaining_input
    from tests.test_gpu_query import _union
    if name == "mid":
        return _genomes(0, MID_GENOMES)
    if name == "mid-last":
        return _genomes(0, MID_GENOMES - 1)
    if name == "mid-two":
        return _genomes(0, MID_GENOMES - 2)
    if name == "mid-middle":
        return tuple(remaining_input(*arrays("mid"), [MIDDLE]))
    base, _, q = name.partition("+")
    return _union(arrays(base), QUERIES[q]())[:3]


class Reference:
    """What the CPU oracle says about one set, read once and left alone; answers like oracle.binding.Oracle."""

    def __init__(self, arrays_, k: int):
        from oracle import binding as ob
        ora = ob.Oracle(*arrays_, k)
        self.arrays, self.k = arrays_, k
        self.genomes, self.sequences, self.total_cost = int(ora.genomes), int(ora.sequences), int(ora.total_cost)
        self.kmer_occurrences = int(ora.kmer_occurrences)
        self._scores = [ora.scores(g) for g in range(self.genomes)]
        self._costs = [int(ora.genome_cost(g)) for g in range(self.genomes)]
        self._dictionary, self.total_visited, self.kseq = ora.dictionary(), ora.total_visited(), ora.kseq_lengths()
        ora.close()

    def scores(self, g):
        return self._scores[g]

    def genome_cost(self, g):
        return self._costs[g]

    def dictionary(self):
        return self._dictionary

    @property
    def cells(self) -> int:
        return sum(int(s["scoresCount"]) for s in self._scores)


@lru_cache(maxsize=None)
def reference(name: str) -> Reference:
    return Reference(arrays(name), mid_k())


@lru_cache(maxsize=None)
def edges(name: str, genome: int):
    """pangenes.bbh_edges on the oracle's block of one genome -> (src, dst, score)"""
    from pandelos_amd.pangenes import bbh_edges
    from pandelos_amd.scores import Scores
    s = reference(name).scores(genome)
    return bbh_edges(Scores(scoresCount=int(s["scoresCount"]), **{f: np.asarray(s[f]) for f in H.FIELDS}))


@lru_cache(maxsize=None)
def network(name: str):
    """(src, dst) of every genome's edges, genome after genome"""
    parts = [edges(name, g) for g in range(reference(name).genomes)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


@lru_cache(maxsize=None)
def families(name: str) -> dict:
    from tests.test_gpu_families import _script_view
    src, dst = network(name)
    gen = arrays(name)[2]
    return _script_view(src, dst, gen.tolist(), len(gen))


@lru_cache(maxsize=None)
def placement(query: str) -> dict:
    """the script's walk of the mid-size set's network plus the held-out genome's edges"""
    from tests.test_place_cpu import script_view
    bs, bd = network("mid")
    gen = arrays("mid")[2]
    qs, qd, _ = edges(f"mid+{query}", MID_GENOMES)
    return script_view(bs, bd, gen.tolist(), len(QUERIES[query]()[1]) - 1, qs, qd)


@lru_cache(maxsize=None)
def profile_case():
    """-> (family_of, genome_of, G, the profile, the two matrices), the last two with numpy"""
    from tests import matrix_cases as MC
    from tests import profile_cases as PC
    f, g, G = PC.random_labelling(PROFILE_SEED, genes=PROFILE_GENES, genomes=PROFILE_GENOMES)
    return f, g, G, PC.profile_numpy(f, g, G), MC.matrices_numpy(f, g, G)


@lru_cache(maxsize=None)
def large_case():
    """-> (digest entry, the set, the 63-genome prefix, the last genome, the set with an intruder in the middle, the intruder's ids)"""
    from tests.test_gpu_append import _genome, _prefix
    from tests.test_gpu_remove import _with_genomes_in_the_middle
    d = json.loads((H.GOLDEN / "digests_baseline.json").read_text())[LARGE]
    gs = H.make_gene_set(**d["shape"])
    G = d["genomes"]
    extra = H.make_gene_set(**{**d["shape"], "genomes": 1, "seed": d["shape"]["seed"] + 77})
    res, off, gen, ids = _with_genomes_in_the_middle(gs, extra, G // 2)
    return (d, gs, _prefix(gs.residues, gs.offsets, gs.genome_of, G - 1), _genome(gs.residues, gs.offsets, gs.genome_of, G - 1, G)[:2],
            (res, off, gen), ids)


# ---- what every scenario shares -----------------------------------------------------------------------------------------------------
def _open(options=()):
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.open()
    for name, v in options:
        nat.set_option(name, v)
    return nat


def _mid_context(options, late):
    from tests.test_gpu_query import _native
    return _native(mid_k(), *arrays("mid"), options=options, late=late)


def _assert_dictionary(nat, ref: Reference, label):
    d = ref.dictionary()
    for got, f in zip(nat.dictionary(), ("rank", "seq", "count")):
        bad = np.flatnonzero(got != d[f])
        assert len(bad) == 0, f"{label}: dictionary {f} differs from the oracle's in {len(bad)} records, first at {int(bad[0])}"


def second_look(nat, ref: Reference, options, label):
    """After a call behind a late switch: the dictionary, the per-gene costs and — the scores dropped by setting the last option
    once more — every genome's block a second time, all against the oracle."""
    _assert_dictionary(nat, ref, f"{label}, second look")
    cost, kl = nat.sequence_costs()
    assert np.array_equal(kl, ref.kseq), f"{label}, second look: k-mers per gene"
    assert np.array_equal(cost, ref.total_visited), f"{label}, second look: per-gene lookups"
    nat.set_option(*options[-1])
    for g in range(ref.genomes):
        H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), ref.scores(g), f"{label}, second look, genome {g}")
        assert nat.genome_cost(g) == ref.genome_cost(g), f"{label}, second look: genome {g} cost"


def _assert_edges(got, want, label):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"{label}: edges differ from bbh_edges on the oracle's block"
    assert H.raw(np.asarray(got[2])).tobytes() == H.raw(np.asarray(want[2])).tobytes(), f"{label}: edge scores differ"


# ---- the scenarios: (options, late, label) ----------------------------------------------------------------------------------------------
def append(options, late=(), label="append"):
    from tests.test_gpu_append import _append_vs_union, _assert_oracle, _assert_same_context
    from tests.test_gpu_query import _native
    k, ends = mid_k(), in_force(options, late)
    last, before_last = held_out(MID_GENOMES - 1), held_out(MID_GENOMES - 2)
    nat = _append_vs_union(arrays("mid-last"), last, k, f"{label}: 8 + 1", options=options, late=late, ora=reference("mid"))
    if late:
        second_look(nat, reference("mid"), ends, f"{label}: 8 + 1")
    nat.close()
    nat = _append_vs_union(arrays("mid-two"), before_last, k, f"{label}: 7 + 1", options=options, late=late, ora=reference("mid-last"))
    nat.append(*last)
    uni = _native(k, *arrays("mid"), options=ends)
    _assert_same_context(nat, uni, f"{label}: 7 + 1 + 1")
    _assert_oracle(nat, *arrays("mid"), k, f"{label}: 7 + 1 + 1", ora=reference("mid"))
    if late:
        second_look(nat, reference("mid"), ends, f"{label}: 7 + 1 + 1")
    uni.close(); nat.close()


def remove(options, late=(), label="remove"):
    from tests.test_gpu_remove import _remove_vs_rebuild
    for removed, rest in (([MIDDLE], "mid-middle"), ([MID_GENOMES - 1], "mid-last")):
        lab = f"{label}: without genome {removed[0]}"
        nat = _remove_vs_rebuild(*arrays("mid"), mid_k(), removed, lab, options=options, late=late, ora=reference(rest))
        if late:
            second_look(nat, reference(rest), in_force(options, late), lab)
        nat.close()


def rekey(options, late=(), label="rekey"):
    """the letter X comes with a genome appended to the mid-size set and goes with it again (option "alphabet_rekey", on before the
    build): every key of more than a look-back chunk of k-mers is written again, then the merge or the compaction and the tail run"""
    from tests import test_gpu_rekey as R
    on = tuple(R.ON) + tuple(options)
    for grown in (True, False):
        if grown:
            lab, ref = f"{label}: + X", reference("mid+x")
            nat = R._append_vs_union(arrays("mid"), QUERIES["x"](), mid_k(), lab, options=on, late=late, ora=ref)
        else:
            lab, ref = f"{label}: - X", reference("mid")
            nat = R._remove_vs_rebuild(*arrays("mid+x"), mid_k(), [MID_GENOMES], lab, options=on, late=late, ora=ref)
        if late:
            second_look(nat, ref, in_force(on, late), lab)
        nat.close()


def query(options, late=(), label="query"):
    from tests.test_gpu_query import _check_against_oracle
    nat = _mid_context(options, late)
    for q in ("9", "big"):
        _check_against_oracle(nat, arrays("mid"), QUERIES[q](), mid_k(), f"{label}: held-out genome {q}", ora=reference(f"mid+{q}"))
    nat.set_option("query_rekey", 1)
    _check_against_oracle(nat, arrays("mid"), QUERIES["x"](), mid_k(), f"{label}: a query with a new letter", ora=reference("mid+x"))
    assert nat.last_query_rekey_info["queries_rekeyed"] == 1, label
    if late:
        second_look(nat, reference("mid"), in_force(options, late), label)
    nat.close()


def query_batch(options, late=(), label="query_batch"):
    nat = _mid_context(options, late)
    names = ("9", "10", "11")
    for budget, chunks in ((None, 1), (1, len(names))):
        if budget:
            nat.set_option("query_batch_bytes", budget)
        blocks = nat.query_batch([QUERIES[q]() for q in names])
        info = nat.last_query_batch_info
        assert info["chunks"] == chunks, f"{label}: {info['chunks']} chunks"
        for j, (q, block) in enumerate(zip(names, blocks)):
            ref = reference(f"mid+{q}")
            H.assert_scores_equal(block.as_dict(), ref.scores(MID_GENOMES), f"{label}: {chunks} chunk(s), query {j}")
            assert info["queries"][j]["genome_cost"] == ref.genome_cost(MID_GENOMES), f"{label}: {chunks} chunk(s), query {j} cost"
    nat.set_option("query_batch_bytes", 1 << 30)
    nat.set_option("query_rekey", 1)
    names = ("9", "x", "11")                                # one chunk whose alphabet is the base's plus the X of its middle query
    blocks = nat.query_batch([QUERIES[q]() for q in names])
    assert nat.last_query_batch_info["chunks"] == 1 and nat.last_query_rekey_info["queries_rekeyed"] == 1, label
    for j, (q, block) in enumerate(zip(names, blocks)):
        H.assert_scores_equal(block.as_dict(), reference(f"mid+{q}").scores(MID_GENOMES), f"{label}: with a new letter in the chunk, query {j}")
    nat.close()


def _assert_placed(pl, q, label, with_edges=True):
    from tests.test_place_cpu import assert_placement
    if with_edges:
        _assert_edges((pl["src"], pl["dst"], pl["score"]), edges(f"mid+{q}", MID_GENOMES), label)
    assert_placement(pl, placement(q), label)


def place(options, late=(), label="place"):
    nat = _mid_context(options, late)
    gen = arrays("mid")[2]
    for q in ("9", "big"):
        _assert_placed(nat.place_query(*QUERIES[q]()), q, f"{label}: held-out genome {q}")
        qs, qd, _ = edges(f"mid+{q}", MID_GENOMES)
        base = nat.families_of_edges(*network("mid"), gen)
        got = nat.placement_of_edges(base, gen, len(QUERIES[q]()[1]) - 1, qs, qd)
        _assert_placed(got, q, f"{label}: the edges of genome {q} handed in", with_edges=False)
    nat.close()


def place_batch(options, late=(), label="place_batch"):
    nat = _mid_context(options, late)
    names = ("9", "10", "11")
    for budget, chunks in ((None, 1), (1, len(names))):
        if budget:
            nat.set_option("query_batch_bytes", budget)
        pls = nat.place_batch([QUERIES[q]() for q in names])
        assert nat.last_place_batch_info["chunks"] == chunks, f"{label}: {nat.last_place_batch_info['chunks']} chunks"
        for j, (q, pl) in enumerate(zip(names, pls)):
            _assert_placed(pl, q, f"{label}: {chunks} chunk(s), query {j}")
    nat.close()


def edges_families(options, late=(), label="edges_families"):
    from tests.test_gpu_families import _assert_same
    nat = _mid_context(options, late)
    ref, gen = reference("mid"), arrays("mid")[2]
    for g in range(ref.genomes):
        _assert_edges(nat.generate_edges_part(g), edges("mid", g), f"{label}: genome {g}")
    _assert_same(nat.generate_families(), families("mid"), f"{label}: pdl_compute_families")
    _assert_same(nat.families_of_edges(*network("mid"), gen), families("mid"), f"{label}: pdl_families_of_edges")
    nat.close()


def profile_matrix(options, late=(), label="profile_matrix"):
    from tests import matrix_cases as MC
    from tests import profile_cases as PC
    f, g, G, want_profile, want_matrices = profile_case()
    nat = _open(in_force(options, late))                    # (neither call needs a build)
    prof = nat.family_profile(f, g, G)
    diff = PC.first_difference(prof, want_profile)
    assert diff is None, f"{label}: profile: {diff}"
    for slab in (None, PROFILE_SLAB_BYTES):
        if slab:
            nat.set_option("matrix_slab_bytes", slab)
        got = nat.genome_matrix(prof)
        diff = MC.first_difference(got, want_matrices)
        assert diff is None, f"{label}: matrices, {got['slabs']} slabs: {diff}"
        assert (got["slabs"] > 2) == bool(slab), f"{label}: {got['slabs']} slabs"
    nat.close()


def batches(options, late=(), label="batches"):
    """scores_in_batches; a late switch falls between the build for batch 0 and the shard of batch 1"""
    ref, ends = reference("mid"), in_force(options, late)
    for per_batch in (1, 3):
        for low_memory in (0, 1):
            lab = f"{label}: batches of {per_batch}, low_memory {low_memory}"
            nat = _open(options)
            seen = 0
            for g, s in nat.scores_in_batches(mid_k(), *ref.arrays, per_batch, low_memory=bool(low_memory)):
                H.assert_scores_equal(s.as_dict(), ref.scores(g), f"{lab}, genome {g}")
                assert nat.genome_cost(g) == ref.genome_cost(g), f"{lab}: genome {g} cost"
                seen += 1
                if g == per_batch - 1:
                    for name, v in late:
                        nat.set_option(name, v)
            assert seen == ref.genomes, lab
            cost, kl = nat.sequence_costs()
            last = ref.arrays[2] >= ref.genomes - per_batch          # (a shard reports the lookups of its own genomes' genes)
            assert np.array_equal(kl, ref.kseq), f"{lab}: k-mers per gene"
            assert np.array_equal(cost[last], ref.total_visited[last]), f"{lab}: per-gene lookups of the last batch"
            if not low_memory:
                _assert_dictionary(nat, ref, lab)
            if late:                                         # the last batch a second time
                nat.set_option(*ends[-1])
                for g in range(ref.genomes - per_batch, ref.genomes):
                    H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), ref.scores(g), f"{lab}, second look, genome {g}")
            nat.close()


def dist(options, late=(), label="dist"):
    from tests.test_gpu_dist import _local
    ref = reference("mid")
    for sender in (True, False):
        lab = f"{label}: 3 ranks, range lists by the {'senders' if sender else 'owners'}"
        lr, cost = _local(3, *ref.arrays, mid_k(), sender_ranges=sender, options=in_force(options, late))
        assert lr.used_sender_ranges == sender, lab
        assert lr.total_cost == ref.total_cost and (cost.sequences, cost.genomes) == (ref.sequences, ref.genomes), lab
        assert [lr.genome_cost(g) for g in range(ref.genomes)] == [ref.genome_cost(g) for g in range(ref.genomes)], lab
        lr.score_all()
        for g in range(ref.genomes):
            H.assert_scores_equal(lr.generate_scores_part(g).as_dict(), ref.scores(g), f"{lab}, genome {g}")
        lr.close()


def large_append_remove(options, late=(), label="large_append_remove"):
    from tests.test_gpu_append import _check_digests
    from tests.test_gpu_query import _native
    d, gs, prefix, last, spliced, ids = large_case()
    nat = _native(d["k"], *prefix, options=options, late=late)
    nat.append(*last)
    assert nat.cost.sequences == d["sequences"] and nat.cost.genomes == d["genomes"], label
    _check_digests(nat, d, f"{label}: 63 + 1")
    nat.close()
    nat = _native(d["k"], *spliced, options=options, late=late)
    nat.remove(ids)
    assert nat.cost.sequences == d["sequences"] and nat.cost.genomes == d["genomes"] and nat.cost.residues == len(gs.residues), label
    _check_digests(nat, d, f"{label}: 64 + 1 - 1")
    nat.close()


SCENARIOS = {"append": append, "remove": remove, "rekey": rekey, "query": query, "query_batch": query_batch, "place": place,
             "place_batch": place_batch, "edges_families": edges_families, "profile_matrix": profile_matrix, "batches": batches,
             "dist": dist, "large_append_remove": large_append_remove}

# every (scenario, form) pair is run, or named here with the reason
NOT_RUN = {("large_append_remove", form): "17 M k-mers take seconds per case: run under the forms whose middle scan launch, radix offsets and record passes differ"
           for form in FORMS if form not in LARGE_FORMS}
# ... and the pairs a form cannot reach (the new file's share of the suite's time): the profile and the matrix run on a context without
# a build or a scoring pass; no placement reads a Scores block through pdl_compute_scores.  (The order_* forms do reach the placements:
# a placement ranks the query's rows with K-order and stands on the base's scoring pass.)
SCORING_ONLY = ("order_wave_per_row", "order_32_lanes", "order_wide_apart", "order_two_scans", "no_host_mirror", "no_stage_timers")
NOT_RUN.update({("profile_matrix", form): "pdl_family_profile and pdl_genome_matrix need no build and no scoring pass: the form cannot reach them"
                for form in SCORING_ONLY})
NOT_RUN.update({(s, "no_host_mirror"): "host_mirror is read by pdl_compute_scores alone, which no placement calls" for s in ("place", "place_batch")})
PAIRS = [(s, f) for s in SCENARIOS for f in FORMS if (s, f) not in NOT_RUN]
LATE_CASES = [(s, f, d) for s in LATE_SCENARIOS for f in LATE_FORMS for d in DIRECTIONS]


def late_options(form: str, direction: str):
    """-> (options before the build, options behind it): "to" the form from the defaults, or "from" it to the defaults"""
    defaults = tuple(DEFAULTS.items())
    return (defaults, FORMS[form]) if direction == "to" else (FORMS[form], defaults)
