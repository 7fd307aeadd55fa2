"""One context carried from one gene set to a DIFFERENT one: smaller, larger, another key width, another input path, another
option, behind a refused call, behind a closed context — everything that outlives pdl_preprocess ("What outlives a build
in a context": grow-only buffers that still hold the larger set, clean flags, look-back words, put-aside lists, valid flags, the
genome shard, the options) meets a set it was not made for.

The tables (which sets, in which order, under which options) and the test that they cover what they are there for are in
tests/test_context_reuse_cpu.py.  The expected value of every step is the reference's own fixture or digest, or the CPU oracle; for
edges, families and placements the host restatements over the ORACLE's blocks.  A fresh context of this library is opened only after
a mismatch, so that the message can say whether the re-use or the set is to blame; it never makes a step pass.  That is also why
_check_case (test_gpu_place), _append_vs_union (test_gpu_append) and _remove_vs_rebuild (test_gpu_remove), which open contexts of their
own and compare with them, have local variants here that take the context and compare with the oracle (Products.place, Products.rest).

"Checked" after a build: the cost block, every genome's cost, the per-gene costs, the dictionary and the rank table; every genome's
Scores block bit for bit and in emission order; the cells per genome against pdl_timings.emitted_cells; scored_rows = the genes of
THIS set; no put-aside entry needed a second look."""
import functools
import hashlib
import types

import numpy as np
import pytest

from pandelos_amd import _lib
from pandelos_amd import place as P
from pandelos_amd.pangenes import bbh_edges
from pandelos_amd.scores import Scores
from tests import helpers as H
from tests import test_context_reuse_cpu as T
from tests.test_gpu_families import _assert_same, _check_against_script, _script_view
from tests.test_gpu_place_batch import check_batch
from tests.test_gpu_query import _check_against_oracle, _union
from tests.test_place_cpu import assert_placement
from tests.test_query_golden import assert_block, load_case

pytestmark = pytest.mark.gpu


# ---- the references -------------------------------------------------------------------------------------------------------------
class Ref:
    """Everything the reference (fixture, digests) and the CPU oracle say about one set; made once, never changed."""

    def __init__(self, spec):
        from oracle import binding as ob
        self.spec = spec
        self.res, self.off, self.gen, self.k = T.load(spec)
        self.arrays = (self.res, self.off, self.gen)
        self.N, self.G, self.M = len(self.gen), int(self.gen.max()) + 1, T.kmer_count(spec)
        kind, _, name = spec.partition(":")
        self.fx = H.load_small(name)[4] if kind == "fx" else None
        self.dg = H.DIGESTS[name] if kind == "dg" else None
        ora = ob.Oracle(self.res, self.off, self.gen, self.k)
        assert ora.status == 0 and ora.genomes == self.G, spec
        self.dictionary, self.total_visited, self.kseq = ora.dictionary(), ora.total_visited(), ora.kseq_lengths()
        self.U = len(self.dictionary)
        self.rank_values, self.last_multiplier, self.rank_base, self.hash_fallback = ora.rank_values, ora.last_multiplier, ora.rank_base, ora.hash_fallback
        self.total_cost, self.genome_cost = int(ora.total_cost), [int(ora.genome_cost(g)) for g in range(self.G)]
        self.want = None if self.dg else [ora.scores(g) for g in range(self.G)]        # (a digest set: the digests are the blocks)
        ora.close()
        self.genes_of = np.bincount(self.gen, minlength=self.G)
        if self.fx is not None:                      # the reference's own numbers where it gives them
            self.total_cost, self.genome_cost = int(self.fx["total_cost"]), [int(x) for x in self.fx["genome_cost"]]
            self.cells = [len(self.fx[f"g{g}_scores"]) for g in range(self.G)]
        elif self.dg is not None:
            self.total_cost, self.genome_cost, self.cells = self.dg["total_cost"], list(self.dg["genome_cost"]), list(self.dg["scoresCount"])
        else:
            self.cells = [int(w["scoresCount"]) for w in self.want]

    @functools.cached_property
    def edges(self):
        """The host's best-hit filter over the oracle's blocks: (src, dst, score) per genome."""
        return [bbh_edges(Scores(scoresCount=int(s["scoresCount"]), **{f: np.asarray(s[f]) for f in H.FIELDS})) for s in self.want]

    @functools.cached_property
    def network(self):
        return np.concatenate([e[0] for e in self.edges]), np.concatenate([e[1] for e in self.edges])

    @functools.cached_property
    def families(self):
        return _script_view(*self.network, self.gen.tolist(), self.N)

    @property
    def gs(self):
        return types.SimpleNamespace(residues=self.res, offsets=self.off, genome_of=self.gen, genes=self.N, genomes=self.G)


@functools.lru_cache(maxsize=None)
def reference(spec):
    return Ref(spec)


def _assert_blocks(ref, blocks, label):
    for g, got in blocks.items():
        assert int(got["scoresCount"]) == ref.cells[g], f"{label}: genome {g} holds {got['scoresCount']} cells, expected {ref.cells[g]}"
        if ref.fx is not None:
            for f in H.FIELDS:
                have, want = H.raw(got[f]), ref.fx[f"g{g}_{f}"]
                assert have.shape == want.shape and np.array_equal(have, want), f"{label}: genome {g} field {f} differs from the fixture"
        elif ref.dg is not None:
            for f in H.FIELDS:
                assert hashlib.sha256(H.raw(got[f]).tobytes()).hexdigest() == ref.dg["sha256"][g][f], f"{label}: genome {g} field {f} digest differs"
        else:
            H.assert_scores_equal(got, ref.want[g], f"{label}: genome {g}")


def _code(fn):
    with pytest.raises(_lib.PdlError) as e:
        fn()
    return e.value.code, str(e.value)


def check_build(nat, ref, label, shard=None, low_memory=False):
    genomes = list(range(ref.G)) if shard is None else list(shard)
    c = nat.cost
    assert (c.sequences, c.genomes, c.kmer_occurrences, c.dictionary_records) == (ref.N, ref.G, ref.M, ref.U), f"{label}: sizes {c.as_dict()}"
    assert (bool(c.hash_fallback), c.rank_base, c.kvalue) == (ref.hash_fallback, ref.rank_base, ref.k), f"{label}: ranking {c.as_dict()}"
    # (a shard's "Total cost" is that of its own genomes: two disjoint shards add up to the set's)
    want_total = ref.total_cost if shard is None else sum(ref.genome_cost[g] for g in genomes)
    assert c.total_cost == want_total, f"{label}: total cost {c.total_cost}, expected {want_total}"
    blocks = {g: nat.generate_scores_part(g).as_dict() for g in genomes}
    _assert_blocks(ref, blocks, label)
    for g in genomes:
        assert nat.genome_cost(g) == ref.genome_cost[g], f"{label}: genome {g} cost"
    for g in sorted(set(range(ref.G)) - set(genomes)):
        assert _code(lambda: nat.generate_scores_part(g))[0] == _lib.PDL_ERR_ARGUMENT, f"{label}: genome {g} is outside the shard"
    counts, tm = nat.scores_counts(), nat.timings()
    assert counts.tolist() == [ref.cells[g] if g in genomes else 0 for g in range(ref.G)], f"{label}: cells per genome {counts.tolist()}"
    assert int(counts.astype(np.int64).sum()) == tm["emitted_cells"], f"{label}: emitted_cells {tm['emitted_cells']}"
    assert tm["scored_rows"] == int(ref.genes_of[genomes].sum()), f"{label}: scored_rows {tm['scored_rows']}, this set has {int(ref.genes_of[genomes].sum())}"
    assert tm["aside_reloads"] == 0 and tm["aside_repeats"] == 0, f"{label}: the put-aside canary went off ({tm['aside_reloads']}, {tm['aside_repeats']})"
    tab, lm = nat.rank_table()
    assert np.array_equal(tab, ref.rank_values) and lm == ref.last_multiplier, f"{label}: rank table"
    if low_memory:
        assert _code(nat.dictionary)[0] == _lib.PDL_ERR_STATE, f"{label}: low_memory keeps no stream"
        return
    ranks, seqs, cnts = nat.dictionary()
    d = ref.dictionary
    assert np.array_equal(ranks, d["rank"]) and np.array_equal(seqs, d["seq"]) and np.array_equal(cnts, d["count"]), f"{label}: dictionary"
    if shard is None:
        cost, kl = nat.sequence_costs()
        assert np.array_equal(cost, ref.total_visited) and np.array_equal(kl, ref.kseq), f"{label}: per-gene costs"


_TINY_QUERY = (np.frombuffer(b"ACDEFGHIKL", np.uint8).copy(), np.array([0, 10], np.uint64))


def assert_refusing(nat, label):
    """Behind a refused build no reader answers — in particular not from the set before it."""
    readers = {"generate_scores_part": lambda: nat.generate_scores_part(0), "generate_edges_part": lambda: nat.generate_edges_part(0),
               "generate_families": nat.generate_families, "query_scores": lambda: nat.query_scores(*_TINY_QUERY),
               "query_batch": lambda: nat.query_batch([_TINY_QUERY]), "place_query": lambda: nat.place_query(*_TINY_QUERY),
               "place_batch": lambda: nat.place_batch([_TINY_QUERY]), "dictionary": nat.dictionary, "score_all": nat.score_all,
               "scores_counts": nat.scores_counts, "genome_cost": lambda: nat.genome_cost(0), "sequence_costs": nat.sequence_costs,
               "rank_table": nat.rank_table, "append": lambda: nat.append(*_TINY_QUERY), "remove": lambda: nat.remove([0])}
    for name, fn in readers.items():
        with pytest.raises(_lib.PdlError) as e:
            fn()
        assert e.value.code == _lib.PDL_ERR_STATE, f"{label}: {name} answered {e.value.code} ({e.value}) behind a refused build"


# ---- one context and what was done to it ----------------------------------------------------------------------------------------
class Run:
    def __init__(self, name, tmp_path=None):
        from pandelos_amd.pangene_native import PangeneNative
        self.name, self.tmp = name, tmp_path
        self.nat = PangeneNative.open()
        self.opts, self.shard, self.history, self.keep, self.built = {}, None, [], None, None

    def close(self):
        self.free_device()
        self.nat.close()

    def label(self, what):
        return f"{self.name}, step {len(self.history)} ({what}); before it: {'; '.join(self.history) or 'nothing'}"

    def done(self, what):
        self.history.append(what)

    def set_options(self, opts):
        for name, value in opts:
            self.nat.set_option(name, value)
            self.opts[name] = value

    def set_shard(self, shard):
        self.nat.set_genome_shard(list(shard))
        self.shard = list(shard) or None

    def free_device(self):
        if self.keep is not None:                    # the device input of the build before: freed before the next one
            import torch
            self.keep = None
            torch.cuda.synchronize()

    def build(self, ref, via="host", only_complexity=False, k=None):
        nat = self.nat
        res, off, gen = ref.arrays
        k = ref.k if k is None else k
        self.free_device()
        self.built = None
        if via == "host":
            nat.preprocess(k, res, off, gen, only_complexity)
        elif via == "device":
            import torch
            dev = torch.device("cuda:0")
            pad = (-len(res)) % 16
            t_res = torch.from_numpy(np.concatenate([res, np.zeros(pad + 16, np.uint8)])).to(dev)
            t_off = torch.from_numpy(off.astype(np.int64)).to(dev)
            t_gen = torch.from_numpy(gen.astype(np.int32)).to(dev)
            torch.cuda.synchronize()
            self.keep = (t_res, t_off, t_gen)
            nat.preprocess_device(k, t_res.data_ptr(), t_off.data_ptr(), t_gen.data_ptr(), len(gen), len(res), only_complexity)
        else:
            assert via == "ingest" and ref.fx is not None
            p = self.tmp / f"step{len(self.history)}.faa"
            p.write_bytes(ref.fx["faa"].tobytes())
            ing = nat.ingest_faa(p)
            assert (ing["sequences"], ing["genomes"], ing["residues"]) == (ref.N, ref.G, len(res)), self.label("ingest")
            nat.preprocess_ingested(k, only_complexity)
        self.built = ref

    def refused(self, fn, code, text, label):
        """A build that must be refused: code, message, and the context answers nothing afterwards."""
        got, msg = _code(fn)
        assert got == getattr(_lib, code) and text in msg, f"{label}: refused with {got} ({msg!r}), expected {code} ({text!r})"
        self.built = None
        assert_refusing(self.nat, label)

    def check(self, ref, label):
        low = bool(self.opts.get("low_memory"))
        try:
            check_build(self.nat, ref, label, self.shard, low)
        except AssertionError as e:
            raise AssertionError(f"{e}\n  -> {self._on_a_fresh_context(ref, low)}") from e

    def _on_a_fresh_context(self, ref, low):
        from pandelos_amd.pangene_native import PangeneNative
        nat = PangeneNative.open()
        try:
            for name, value in self.opts.items():
                nat.set_option(name, value)
            if self.shard:
                nat.set_genome_shard(self.shard)
            nat.preprocess(ref.k, *ref.arrays)
            check_build(nat, ref, "fresh", self.shard, low)
            return "right on a fresh context: re-use"
        except AssertionError:
            return "also wrong on a fresh context"
        except Exception as e:                       # noqa: BLE001 (the verdict is a courtesy: the step has failed already)
            return f"a fresh context fails otherwise: {e!r}"
        finally:
            nat.close()

    # -- a step of a ladder (test_context_reuse_cpu.step) --
    def step(self, st):
        ref = reference(st["spec"])
        what = st["spec"] + "".join(f", {n} = {v}" for n, v in st["opts"]) + (f", via {st['via']}" if st["via"] != "host" else "") + \
            (", only_complexity" if st["only_complexity"] else "") + (f", shard {list(st['shard'])}" if st["shard"] is not None else "") + \
            (f", k = {st['k']}" if st["k"] is not None else "") + (f", must be refused: {st['expect'][0]}" if st["expect"] else "")
        label = self.label(what)
        self.set_options(st["opts"])
        if st["shard"] is not None:
            self.set_shard(st["shard"])
        if st["expect"]:
            self.refused(lambda: self.build(ref, st["via"], st["only_complexity"], st["k"]), *st["expect"], label)
        else:
            self.build(ref, st["via"], st["only_complexity"], st["k"])
            if st["only_complexity"]:
                c = self.nat.cost
                assert (c.sequences, c.genomes, c.kmer_occurrences, c.dictionary_records, c.total_cost) == (ref.N, ref.G, ref.M, ref.U, ref.total_cost), label
                assert _code(lambda: self.nat.generate_scores_part(0))[0] == _lib.PDL_ERR_STATE, label
                assert _code(self.nat.generate_families)[0] == _lib.PDL_ERR_STATE, label
            else:
                self.check(ref, label)
                tm = self.nat.timings()
                for field, least in st["takes"].items():
                    assert tm[field] >= least, f"{label}: {field} = {tm[field]}: the step does not take the path it is there for"
        self.done(what)


# ---- A. ladders -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(T.LADDERS))
def test_ladder(name, tmp_path):
    run = Run(f"ladder {name}", tmp_path)
    for st in T.LADDERS[name]:
        run.step(st)
    run.close()


# -- 5. derived products across a rebuild --
def _block(want):
    return Scores(scoresCount=int(want["scoresCount"]), **{f: np.asarray(want[f]) for f in H.FIELDS})


class Products:
    """One base, one newcomer, and every derived product of the context checked as its own test file checks it — against the
    oracle's blocks, the host's filter and the host restatements over them."""

    def __init__(self, base_spec, union_spec, query, fixture=None):
        self.base, self.union, self.query, self.fx = reference(base_spec), reference(union_spec), query, fixture
        self.G, self.n = self.base.G, len(query[1]) - 1
        self.q_edges = bbh_edges(_block(self.union.want[self.G]))
        self.placement = P.placement_from_edges(*self.base.network, self.base.gen, self.n, self.q_edges[0], self.q_edges[1])

    def families(self, nat, label):
        _assert_same(nat.generate_families(), self.base.families, f"{label}: families")

    def edges(self, nat, label):
        for g in range(self.G):
            src, dst, sc = nat.generate_edges_part(g)
            w = self.base.edges[g]
            assert np.array_equal(src, w[0]) and np.array_equal(dst, w[1]) and H.raw(sc).tobytes() == H.raw(w[2]).tobytes(), f"{label}: edges of genome {g}"

    def place(self, nat, label):
        pl = nat.place_query(*self.query)
        src, dst, score = self.q_edges
        assert np.array_equal(pl["src"], src) and np.array_equal(pl["dst"], dst) and H.raw(pl["score"]).tobytes() == H.raw(score).tobytes(), f"{label}: the newcomer's edges"
        assert_placement(pl, self.placement, f"{label}: placement")
        assert pl["sequences"] == self.base.N and pl["genomes"] == self.G, label

    def query_block(self, nat, label):
        got = nat.query_scores(*self.query).as_dict()
        H.assert_scores_equal(got, self.union.want[self.G], f"{label}: query")
        assert nat.last_query_info["genome_cost"] == self.union.genome_cost[self.G], label
        if self.fx is not None:
            assert_block(got, self.fx, f"{label}: query against the fixture")

    FIRST = {"generate_families": families, "generate_edges_part": edges, "place_query": place, "query_scores": query_block}

    def rest(self, run, label):
        nat, base, union = run.nat, self.base, self.union
        for name, reader in self.FIRST.items():
            reader(self, nat, f"{label}, {name}")
        _check_against_script(nat, base.gs, f"{label}: families against the script over the context's own edges")
        _check_against_oracle(nat, base.arrays, self.query, base.k, f"{label}: query against the oracle on the union")
        rq, oq = self.query
        h = max(1, self.n // 2)
        half = (rq[:int(oq[h])].copy(), oq[:h + 1].copy())
        blocks = nat.query_batch([self.query, half, self.query])
        from oracle import binding as ob
        ur, uo, ug, G = _union(base.arrays, half)
        ora = ob.Oracle(ur, uo, ug, base.k)
        for j, want in enumerate((union.want[self.G], ora.scores(G), union.want[self.G])):
            H.assert_scores_equal(blocks[j].as_dict(), want, f"{label}: query_batch, query {j}")
        check_batch(nat, base.gen, [self.query, half], f"{label}: place_batch", base_edges=base.network)
        _assert_same(nat.families_of_edges(*base.network, base.gen), base.families, f"{label}: families_of_edges")
        assert_placement(nat.placement_of_edges(base.families, base.gen, self.n, self.q_edges[0], self.q_edges[1]), self.placement, f"{label}: placement_of_edges")
        self.place(nat, f"{label}, place_query behind the caller's lists")
        run.check(base, f"{label}: the base behind its products")
        # append the newcomer: the union's context; remove it again: the base's
        nat.append(*self.query)
        info = nat.last_append_info
        assert info["residues"] == len(rq) and info["records"] == union.U - base.U and info["kmer_occurrences"] == union.M - base.M, f"{label}: append info {info}"
        run.check(union, f"{label}: behind the append")
        for g in range(union.G):
            src, dst, sc = nat.generate_edges_part(g)
            w = union.edges[g]
            assert np.array_equal(src, w[0]) and np.array_equal(dst, w[1]) and H.raw(sc).tobytes() == H.raw(w[2]).tobytes(), f"{label}: edges of genome {g} behind the append"
        _assert_same(nat.generate_families(), union.families, f"{label}: families behind the append")
        nat.remove([self.G])
        info = nat.last_remove_info
        assert (info["sequences"], info["residues"], info["kmer_occurrences"], info["records"]) == (self.n, len(rq), union.M - base.M, union.U - base.U), f"{label}: remove info {info}"
        run.check(base, f"{label}: behind the removal")
        self.families(nat, f"{label}, behind the removal")
        self.place(nat, f"{label}, behind the removal")


def _ladder5_products():
    name = T.LADDER5[0].partition(":")[2]
    fx, _, query, _, _ = load_case(name)
    rq, oq, _ = query.flatten()
    x = Products(T.LADDER5[0], "qu:" + name, (rq, oq), fx)
    y = Products(T.LADDER5[1], T.LADDER5_Y + "|union", T.held(T.LADDER5_Y))
    return x, y


@pytest.mark.parametrize("first", sorted(Products.FIRST))
def test_ladder_5_derived_products_across_a_rebuild(first):
    """X with every product, then Y: `first` is the very first call behind pdl_preprocess — no scoring call in between, the mirror,
    the edges and the families of X still lie in the context — then the rest, then X again the same way."""
    x, y = _ladder5_products()
    run = Run(f"ladder 5, first reader {first}")
    for name, pr in (("X", x), ("Y", y), ("X again", x)):
        what = f"{name} = {pr.base.spec}"
        label = run.label(what)
        run.build(pr.base)
        if name != "X":
            Products.FIRST[first](pr, run.nat, f"{label}, {first} as the first call behind the build")
        pr.rest(run, label)
        run.done(what + ", every product, append, remove")
    run.close()


# -- 6. failed calls between builds --
@pytest.mark.parametrize("failure", T.FAILURES)
def test_ladder_6_a_failed_call_between_two_builds(failure):
    x_spec = T.LADDER6_REMOVE if failure == "refused_remove" else T.LADDER6[0]
    x, y = reference(x_spec), reference(T.LADDER6[1])
    run = Run(f"ladder 6, {failure}")
    nat = run.nat
    run.step(T.step(x_spec))
    label = run.label(failure)
    res, off, gen = x.arrays
    if failure == "k_is_0":
        run.refused(lambda: nat.preprocess(0, res, off, gen), "PDL_ERR_KVALUE", "K value must be greater than 0", label)
    elif failure == "k_is_500":
        run.refused(lambda: nat.preprocess(500, res, off, gen), "PDL_ERR_EMPTY", "no gene is at least k=500 residues long", label)
    elif failure == "no_gene":
        run.refused(lambda: nat.preprocess(x.k, np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32)), "PDL_ERR_EMPTY", "empty dataset", label)
    elif failure == "genome_ids_not_dense":
        r4 = reference("fx:readme4_k2")
        run.refused(lambda: nat.preprocess(r4.k, r4.res, r4.off, np.array([0, 9, 0, 9], np.uint32)), "PDL_ERR_ARGUMENT", "genome ids are not dense", label)
    elif failure == "refused_append":
        code, msg = _code(lambda: nat.append(np.frombuffer(b"ACAZZ", np.uint8), np.array([0, 5], np.uint64)))
        assert code == _lib.PDL_ERR_UNSUPPORTED and "0x5a" in msg, f"{label}: {code} {msg!r}"
        code, msg = _code(lambda: nat.append(res[:40].copy(), np.array([0, 40], np.uint64), np.array([x.G + 1], np.uint32)))
        assert code == _lib.PDL_ERR_ARGUMENT and "not dense" in msg, f"{label}: {code} {msg!r}"
        run.check(x, f"{label}: X behind the refused appends")
    else:
        code, msg = _code(lambda: nat.remove([x.G - 1]))                   # the genome that alone holds Z: found out on the device
        assert code == _lib.PDL_ERR_UNSUPPORTED and "0x5a" in msg, f"{label}: {code} {msg!r}"
        code, msg = _code(lambda: nat.remove([x.G]))
        assert code == _lib.PDL_ERR_ARGUMENT and "out of range" in msg, f"{label}: {code} {msg!r}"
        run.check(x, f"{label}: X behind the refused removals")
    run.done(failure)
    run.step(T.step(T.LADDER6[1]))
    assert y.N != x.N
    run.close()


# -- 7. across contexts --
def test_ladder_7_a_closed_context_and_the_next_ones():
    """A context that scored the large set under a filter tier is closed; two new ones are opened at once on small sets: the device
    memory they are given is what the first one left (put-aside lists, tables, look-back words), which the launch serial and the
    clean flags of the NEW contexts must not trust."""
    big, small = T.LADDER7[0], T.LADDER7[1:]
    for tier in (10, 11, 21):
        a = Run(f"ladder 7, tier {tier}, the closed context")
        a.step(T.step(big, opts=(("join_tier1", tier),)))
        a.close()
        runs = [Run(f"ladder 7, tier {tier}, new context {i} behind the closed one") for i in range(2)]
        for _ in range(2):                                                  # each of the two takes both small sets, in opposite order
            for run, spec in zip(runs, small):
                run.step(T.step(spec, opts=(("join_tier1", tier),)))
            small = small[::-1]
        for run in runs:
            run.close()


# ---- B. random walks ----------------------------------------------------------------------------------------------------------------
def _walk_step(run, st):
    nat = run.nat
    spec = T.built_spec(st)
    res, off, gen, k = T.load(spec)
    G = int(gen.max()) + 1
    every_other = list(range(0, G, 2))
    what = f"{spec}, change {st['change']}, action {st['action']}" + (", holds no k-mer" if st["empty"] else "")
    label = run.label(what)
    if st["change"] is not None:
        name, value = st["change"]
        if name != "shard":
            run.set_options([(name, value)])
        else:
            if run.built is not None:               # a built context takes another shard only behind a refused build
                run.refused(lambda: nat.preprocess(0, res, off, gen), "PDL_ERR_KVALUE", "K value must be greater than 0", f"{label}: k = 0 in front of the shard change")
            run.set_shard(every_other if value else ())
    if run.shard and max(run.shard) >= G:           # the shard of an earlier set stays in force: it names genomes this set lacks
        run.refused(lambda: nat.preprocess(k, res, off, gen), "PDL_ERR_ARGUMENT", "genome shard: id", f"{label}: the stale shard {run.shard}")
        run.set_shard(every_other)
    if st["empty"]:
        run.refused(lambda: nat.preprocess(k, res, off, gen), "PDL_ERR_EMPTY", "the dictionary is empty", label)
        run.done(what)
        return
    ref = reference(spec)
    run.build(ref)
    run.check(ref, label)
    low, shard = bool(run.opts.get("low_memory")), run.shard
    action = st["action"]
    if action == "families":
        if shard:
            code, msg = _code(nat.generate_families)
            assert code == _lib.PDL_ERR_STATE and "shard" in msg, f"{label}: families under a shard: {code} {msg!r}"
        else:
            for g in range(ref.G):
                src, dst, sc = nat.generate_edges_part(g)
                w = ref.edges[g]
                assert np.array_equal(src, w[0]) and np.array_equal(dst, w[1]) and H.raw(sc).tobytes() == H.raw(w[2]).tobytes(), f"{label}: edges of genome {g}"
            _assert_same(nat.generate_families(), ref.families, f"{label}: families")
            _check_against_script(nat, ref.gs, f"{label}: families against the script")
    elif action in ("query", "append_remove"):
        query = T.held(st["spec"])
        union = reference(st["spec"] + "|union")
        if action == "query":
            if low:
                code, msg = _code(lambda: nat.query_scores(*query))
                assert code == _lib.PDL_ERR_STATE and "low_memory" in msg, f"{label}: query under low_memory: {code} {msg!r}"
            else:
                got, _ = _check_against_oracle(nat, ref.arrays, query, k, f"{label}: query")
                H.assert_scores_equal(got, union.want[ref.G], f"{label}: query")
        elif shard or low:
            for fn in (lambda: nat.append(*query), lambda: nat.remove([0])):
                code, msg = _code(fn)
                assert code == _lib.PDL_ERR_STATE and ("shard" if shard else "low_memory") in msg, f"{label}: {code} {msg!r}"
            run.check(ref, f"{label}: behind the refused append and removal")
        else:
            nat.append(*query)
            run.built = union
            run.check(union, f"{label}: behind the append")
            nat.remove([ref.G])
            run.built = ref
            run.check(ref, f"{label}: behind the removal")
    run.done(what)


@pytest.mark.parametrize("seed", T.walk_seeds())
def test_random_walk(seed):
    run = Run(f"walk {seed}")
    for st in T.walk(seed):
        _walk_step(run, st)
    run.close()
