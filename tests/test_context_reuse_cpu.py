"""The tables behind tests/test_gpu_context_reuse.py — which sets one context is carried through, under which options, in which
order — and one test of those tables that needs no GPU: a ladder that does not change N, G, M and U between two builds, a key-kind
walk that misses a transition, or sixteen random walks that never shrink a set, never draw an option or never meet a set without a
k-mer would leave the state that outlives a build ("What outlives a build in a context") unexercised without any test
failing.

A set is named by a spec string; `load(spec)` makes its arrays (numpy only):
    fx:NAME             tests/golden/NAME.npz, the reference's own fixture
    dg:NAME             a set of tests/golden/digests.json, pinned by the reference's digests
    qb:NAME / qu:NAME   the base part / the union of the query fixture tests/golden/query/NAME.npz
    fz:SEED             test_gpu_fuzz._random_set(SEED)
    mk:G:P:L:SUB:SEED:K make_gene_set(G genomes, P genes per genome, mean length L, SUB % substitutions, SEED) at k = K
    big330              the 330-genome set of test_more_than_320_genomes_take_the_2048_slot_tier_and_match_the_oracle
    az:NAME             fixture NAME and one more genome that alone holds the letter Z (its removal is refused on the device)
and three suffixes: "|base" is the set without its last genome (`held(spec)` is that genome, as a query), "|union" that base with
the held genome's genes behind it (what an append of it leaves), "|kmax" the same arrays at k = longest gene + 1: a set in which
no gene holds a k-mer."""
import functools
import os

import numpy as np

from tests import helpers as H
from tests.test_gpu_fuzz import _random_set
from tests.test_gpu_query import _split
from tests.test_remove_cpu import classify_removal

KINDS = ("32", "64", "hash")                 # 32-bit keys, 64-bit keys, hashed ranks (64-bit keys of another ranking)
BIG330 = dict(genomes=330, genes_per_genome=36, mean_len=90, sub_rate=0.1, seed=3301)


def _plain(spec):
    kind, _, arg = spec.partition(":")
    if kind == "fx":
        return H.load_small(arg)[:4]
    if kind == "dg":
        return H.load_large(arg)[:4]
    if kind in ("qb", "qu"):
        from tests.test_query_golden import load_case, union_arrays
        fx, base, query, k, G = load_case(arg)
        return (*base.flatten(), k) if kind == "qb" else (*union_arrays(base, query)[:3], k)
    if kind == "fz":
        return _random_set(int(arg))
    if kind == "mk":
        g, p, l, sub, seed, k = (int(x) for x in arg.split(":"))
        gs = H.make_gene_set(genomes=g, genes_per_genome=p, mean_len=l, sub_rate=sub / 100.0, seed=seed)
        return gs.residues, gs.offsets, gs.genome_of, k
    if kind == "big330":
        from pandelos_amd.calculate_k import calculate_k
        gs = H.make_gene_set(**BIG330)
        return gs.residues, gs.offsets, gs.genome_of, calculate_k(gs.residues)
    if kind == "az":
        res, off, gen, k = H.load_small(arg)[:4]
        extra = np.frombuffer(b"ZZZZZZ" + res[:40].tobytes(), np.uint8)
        return (np.concatenate([res, extra]), np.append(off, off[-1] + np.uint64(len(extra))).astype(np.uint64),
                np.append(gen, np.uint32(int(gen.max()) + 1)).astype(np.uint32), k)
    raise KeyError(spec)


@functools.lru_cache(maxsize=None)
def load(spec):
    """-> (residues, offsets, genome_of, k); the arrays are shared: never change them"""
    name, *suffixes = spec.split("|")
    res, off, gen, k = _plain(name)
    res, off, gen = np.ascontiguousarray(res, np.uint8), np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(gen, np.uint32)
    for s in suffixes:
        if s == "base":
            res, off, gen = _split(res, off, gen, int(gen.max()))[0]
        elif s == "union":
            from tests.test_gpu_query import _union
            res, off, gen = _union(*_split(res, off, gen, int(gen.max())))[:3]
        elif s == "kmax":
            k = int(np.diff(off.astype(np.int64)).max(initial=0)) + 1
        else:
            raise KeyError(spec)
    return res, off, gen, int(k)


def held(spec):
    """The last genome of `spec`, which spec + "|base" leaves out: (residues, offsets) of a query."""
    res, off, gen, _ = load(spec)
    return _split(res, off, gen, int(gen.max()))[1]


def kmer_count(spec):
    _, off, _, k = load(spec)
    return int(np.maximum(np.diff(off.astype(np.int64)) - k + 1, 0).sum())


def holds_no_kmer(spec):
    return kmer_count(spec) == 0


@functools.lru_cache(maxsize=None)
def counts(spec):
    """(N genes, G genomes, M k-mer occurrences, U dictionary records, key kind), U and the kind from the CPU oracle"""
    from oracle import binding as ob
    res, off, gen, k = load(spec)
    ora = ob.Oracle(res, off, gen, k, only_complexity=True)
    assert ora.status == 0, spec
    kind = "hash" if ora.hash_fallback else ("64" if ora.rank_base ** k > 1 << 32 else "32")
    out = (len(gen), int(gen.max()) + 1, kmer_count(spec), len(ora.dictionary()), kind)
    ora.close()
    return out


def step(spec, **kw):
    """One build of a ladder.  opts: options set before it; via: "host", "device" or "ingest"; only_complexity; shard: None leaves
    the context's shard alone, a list sets it, () clears it; k: another k than the set's; expect: (error code name, text of the
    message) of a build that must be refused; takes: {field of pdl_timings: least value} — the tier the step is there for."""
    return dict({"spec": spec, "opts": (), "via": "host", "only_complexity": False, "shard": None, "k": None, "expect": None, "takes": {}}, **kw)


BIG, MID = "dg:synth_16x1000x300_k5", "dg:synth_40x60x40_k3"
# k = 2: every gene shares a k-mer with nearly every other one, a row's candidates are the genes above it, and the tiny second-tier
# table holds 384 of them: the upper rows of a set of more than 385 genes can only be scored by the HBM-table kernel (tier 3),
# and with the tiny table off the rows of more than 1024 candidates leave the filter tier's 1024 slots for tier 2
DENSE_1500, DENSE_720 = "mk:10:150:60:30:205:2", "mk:6:120:60:30:207:2"
SHARD_REFUSAL = ("PDL_ERR_ARGUMENT", "genome shard: id 3 out of range (2 genomes)")
LADDER1 = [BIG, "fx:readme4_k1", "fx:synth_5x60x80_k3", MID, "fx:readme4_k3", "fx:short_and_duplicate_genes", BIG]
# every ordered pair of key kinds once: 32 32 64 64 hash hash 32 hash 64 32
LADDER2 = ["fx:synth_5x60x80_k3", "fx:readme4_k2", "fx:synth_5x60x80_k13", "fz:3003", "fx:synth_5x60x80_k16_hash",
           "qu:hash_fallback_20_letters_k16", "fx:synth_5x60x80_k3", "fz:3010", "fx:synth_5x60x80_k14", "fx:readme4_k2"]
LADDERS = {
    "1_shrink_and_grow": [step(s) for s in LADDER1],
    "1_shrink_and_grow_tier0": [step(s, opts=(("join_tier0", 1),)) for s in LADDER1],
    "2_key_kinds_lean_radix": [step(s, opts=(("lean_radix", 1),)) for s in LADDER2],
    "2_key_kinds_full_radix": [step(s, opts=(("lean_radix", 0),)) for s in LADDER2],
    # a shard that outlives its set: refused before a kernel (host input) and from inside the pipeline (device input); a built
    # context takes another shard only behind a refused build, which is how the ladder gets from one to the next
    "3_shard": [step("fx:synth_5x60x80_k3", shard=[1, 3]),
                step("fx:readme4_k2", expect=SHARD_REFUSAL),
                step("fx:readme4_k2", shard=()),
                step("fx:synth_5x60x80_k13", k=0, expect=("PDL_ERR_KVALUE", "K value must be greater than 0")),
                step("fx:synth_5x60x80_k13", shard=[1, 3], via="device"),
                step("fx:readme4_k1", via="device", expect=SHARD_REFUSAL),
                step("fx:low_complexity", shard=(), via="device"),
                step(MID)],
    "3_complexity_and_low_memory": [step("fx:synth_5x60x80_k3", only_complexity=True),
                                    step(MID),
                                    step("fx:low_complexity", opts=(("low_memory", 1),)),
                                    step("dg:synth_8x300x200_k4_div25", opts=(("low_memory", 0),)),
                                    step("fx:synth_5x60x80_k14", opts=(("low_memory", 1),)),
                                    step(MID, only_complexity=True),
                                    step("fx:readme4_k3", opts=(("low_memory", 0),))],
    "3_input_paths": [step(MID), step("fx:synth_5x60x80_k3", via="device"), step("fx:interleaved_genomes", via="ingest"),
                      step("dg:synth_8x300x200_k4_div25"), step("fx:synth_5x60x80_k16_hash", via="device"),
                      step("fx:readme4_k2", via="ingest"), step("fx:short_and_duplicate_genes", via="device"), step(MID)],
    # the largest first and again last; in between the look-back words meet a set of one tile behind one of thousands
    "4_onepass_scan": [step(BIG, opts=(("onepass_scan", 0),)), step("fx:readme4_k1", opts=(("onepass_scan", 1),)),
                       step(MID, opts=(("onepass_scan", 1),)), step(BIG, opts=(("onepass_scan", 0),)),
                       step("fx:low_complexity", opts=(("onepass_scan", 1),)), step(BIG), step("fx:readme4_k3"),
                       step(MID, opts=(("onepass_scan", 0),))],
    "4_join_tier1": [step(s, opts=(("join_tier1", t),), takes={"tier2_rows": 1} if t == 0 else {}) for s, t in zip(
        [MID, "fx:synth_5x60x80_k3", "dg:synth_8x300x200_k4_div25", "fx:low_complexity", "dg:protein_like_12x400x150_k4_div30",
         "fx:short_and_duplicate_genes", BIG], [0, 9, 10, 11, 20, 21, -1])],
    "4_more_than_320_genomes": [step("fx:readme4_k2"), step("big330"), step("fx:interleaved_genomes"), step("big330"),
                                step("fx:synth_5x60x80_k3")],
    # ... then tier 3 for real: its tables, "left zeroed", are laid out by N — 1500 genes, 4, 720, and the tier off again
    "4_tiny_tier2": [step("fx:low_complexity", opts=(("join_tiny_tier2", 1),)), step(BIG), step("fx:readme4_k1"),
                     step(DENSE_1500, takes={"overflow_rows": 1}), step("fx:readme4_k2"), step(DENSE_720, takes={"overflow_rows": 1}),
                     step("qb:protein_like_held_out", opts=(("join_tiny_tier2", 0),)), step(DENSE_1500, takes={"tier2_rows": 1})],
    "4_staging_cap": [step(MID), step("fx:synth_5x60x80_k3", opts=(("staging_cap", 16),), takes={"join_launches": 6}),      # (a pass queues the three tiers; twice)
                      step("fx:low_complexity", takes={"join_launches": 6}),
                      step("dg:synth_8x300x200_k4_div25", opts=(("staging_cap", 0),))],
}
# ladders 5-7 are written out in the GPU file; the sets they move between:
LADDER5 = ("qb:protein_like_held_out", "mk:7:60:90:20:4242:3|base")               # X (its query: the fixture's), Y (its query: held(...))
LADDER5_Y = "mk:7:60:90:20:4242:3"
LADDER6 = ("fx:synth_5x60x80_k3", MID)                                              # X, Y
LADDER6_REMOVE = "az:synth_5x60x80_k3"                                              # X of the refused removal
LADDER7 = (BIG, "fx:readme4_k1", "fx:synth_5x60x80_k3")
FAILURES = ("k_is_0", "k_is_500", "no_gene", "genome_ids_not_dense", "refused_append", "refused_remove")


# ---- random walks ---------------------------------------------------------------------------------------------------------------
WALK_SEED0 = 100
WALK_SEEDS_DEFAULT = 16
WALK_STEPS = 8
OPTION_CHANGES = ("none", "join_tier1", "join_tier0", "join_tiny_tier2", "onepass_scan", "lean_radix", "low_memory", "shard")
ACTIONS = ("score", "families", "query", "append_remove")


def _usable(spec, action):
    """Whether `action` can be checked on `spec` (numpy only, decided where the walk is drawn: no step is skipped when it runs)."""
    res, off, gen, k = load(spec)
    if action in ("score", "families"):
        return True
    if len(gen) == 0 or int(gen.max()) < 1:
        return False                                                      # one genome: nothing to hold out
    (rb, ob_, gb), (rq, oq) = _split(res, off, gen, int(gen.max()))
    if int((np.diff(ob_.astype(np.int64)) >= k).sum()) == 0 or not np.isin(rq, rb).all():
        return False                                                      # no base k-mer / a letter the base lacks: refused
    from tests.test_gpu_query import _union
    ur, uo, ug, G = _union((rb, ob_, gb), (rq, oq))
    return action == "query" or classify_removal(ur, uo, ug, k, [G]) == "ok"


def walk(seed):
    """Eight steps: {"spec", "change": (option, value) or None, "action", "empty"}.  A "shard" change turns the genome shard on
    (every other genome of the step's set) or off; a step whose set holds no k-mer ("empty") must be refused with PDL_ERR_EMPTY.
    For "query" and "append_remove" the context is built on spec + "|base" and the last genome comes as the newcomer."""
    rng = np.random.default_rng(seed)
    state = {"join_tiny_tier2": 0, "onepass_scan": 0, "lean_radix": 1, "low_memory": 0, "shard": 0}
    steps = []
    for _ in range(WALK_STEPS):
        change = OPTION_CHANGES[int(rng.integers(len(OPTION_CHANGES)))]
        action = ACTIONS[int(rng.integers(len(ACTIONS)))]
        empty = bool(rng.random() < 1 / 12)
        while True:                                                       # (the next draw where the action cannot be checked on this one)
            if rng.random() < 0.5:
                spec = f"fz:{int(rng.integers(3000, 3400))}"
            else:
                spec = (f"mk:{int(rng.integers(2, 13))}:{int(rng.integers(5, 201))}:{int(rng.integers(30, 121))}:"
                        f"{int(rng.choice([2, 8, 20]))}:{int(rng.integers(1, 1000))}:{int(rng.choice([3, 4]))}")
            if empty or _usable(spec, action):
                break
        if empty:
            spec, action = spec + "|kmax", "score"
        if change == "none":
            ch = None
        elif change == "join_tier1":
            ch = (change, int(rng.choice([-1, 0, 9, 10, 11, 20, 21])))
        elif change == "join_tier0":
            ch = (change, int(rng.choice([-1, 0, 1])))
        else:
            state[change] ^= 1
            ch = (change, state[change])
        steps.append({"spec": spec, "change": ch, "action": action, "empty": empty})
    return steps


def walk_seeds():
    return list(range(WALK_SEED0, WALK_SEED0 + int(os.environ.get("PDL_REUSE_SEEDS", str(WALK_SEEDS_DEFAULT)))))


def built_spec(st):
    return st["spec"] + "|base" if st["action"] in ("query", "append_remove") else st["spec"]


# ---- the test of the tests ------------------------------------------------------------------------------------------------------
def test_the_ladders_and_the_default_walks_cover_what_they_are_there_for():
    # ladder 2: every ordered pair of key kinds, a kind behind itself included, under both radix settings
    for name in ("2_key_kinds_lean_radix", "2_key_kinds_full_radix"):
        kinds = [counts(st["spec"])[4] for st in LADDERS[name]]
        assert set(zip(kinds, kinds[1:])) == {(a, b) for a in KINDS for b in KINDS}, (name, kinds)
        assert kinds[0] == kinds[-1] and len(kinds) == 10, (name, kinds)          # nine transitions, one closed walk
    assert {st["opts"] for st in LADDERS["2_key_kinds_lean_radix"]} == {(("lean_radix", 1),)}
    assert {st["opts"] for st in LADDERS["2_key_kinds_full_radix"]} == {(("lean_radix", 0),)}
    # every ladder: two builds in a row differ in N, G, M and U (a refused build has no set: the sets on either side of it count)
    sequences = {name: [st["spec"] for st in steps if not st["expect"]] for name, steps in LADDERS.items()}
    sequences.update({"5": [LADDER5[0], LADDER5[1], LADDER5[0]], "6": list(LADDER6), "6_remove": [LADDER6_REMOVE, LADDER6[1]],
                      "7": [LADDER7[0], LADDER7[1], LADDER7[2], LADDER7[0]]})
    for name, specs in sequences.items():
        for a, b in zip(specs, specs[1:]):
            ca, cb = counts(a), counts(b)
            assert all(x != y for x, y in zip(ca[:4], cb[:4])), f"ladder {name}: {a} {ca} -> {b} {cb} keeps one of N, G, M, U"
    assert counts(LADDERS["3_shard"][0]["spec"])[1] == 5 and counts(LADDERS["3_shard"][1]["spec"])[1] == 2       # "id 3 out of range (2 genomes)"
    assert counts(LADDERS["3_shard"][4]["spec"])[1] == 5 and counts(LADDERS["3_shard"][5]["spec"])[1] == 2
    assert {st["opts"][0][1] for st in LADDERS["4_join_tier1"]} == {0, 9, 10, 11, 20, 21, -1}
    assert counts("big330")[1] > 320 and counts(DENSE_1500)[0] > 1024 + 300 and counts(DENSE_720)[0] > 385 + 300
    assert LADDER5_Y + "|base" == LADDER5[1] and classify_removal(*load(LADDER6_REMOVE), [5]) == "alphabet"
    # the default walks between them
    steps = [st for seed in range(WALK_SEED0, WALK_SEED0 + WALK_SEEDS_DEFAULT) for st in walk(seed)]
    assert len(steps) == WALK_SEEDS_DEFAULT * WALK_STEPS
    changes = {"none" if st["change"] is None else st["change"][0] for st in steps}
    assert changes == set(OPTION_CHANGES), sorted(set(OPTION_CHANGES) - changes)
    assert {st["change"][1] for st in steps if st["change"] and st["change"][0] == "shard"} == {0, 1}              # on and off
    assert {st["action"] for st in steps} == set(ACTIONS)
    assert sum(st["empty"] for st in steps) >= 1 and all(holds_no_kmer(built_spec(st)) == st["empty"] for st in steps)
    shrinks = grows = 0
    for seed in range(WALK_SEED0, WALK_SEED0 + WALK_SEEDS_DEFAULT):
        m = [kmer_count(built_spec(st)) for st in walk(seed) if not st["empty"]]
        shrinks += sum(4 * b <= a for a, b in zip(m, m[1:]))
        grows += sum(b >= 4 * a for a, b in zip(m, m[1:]))
        for st in walk(seed):
            sp = built_spec(st)
            if not st["empty"]:
                n, g, mm = len(load(sp)[2]), int(load(sp)[2].max()) + 1, kmer_count(sp)
                assert g <= 12 and mm <= 12 * 200 * 240, (seed, sp, n, g, mm)                     # small sets only: the walks stay quick
    assert shrinks >= 1 and grows >= 1, (shrinks, grows)
