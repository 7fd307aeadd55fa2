"""``PangeneNative`` — host-side mirror of ``ig/infoasys/cli/pangenes/PangeneNative.java`` over the C ABI.

Same surface as the Java class: the constructor preprocesses (PangeneNative.java:5-7),
``print_complexity`` is the ``-c`` mode (:10-12), ``generate_scores_part(genome, multithread)``
returns one ``Scores`` block (:17-21).  Underneath are ``pdl_preprocess`` / ``pdl_compute_scores``
of ``include/pandelos_amd.h``; errors come back as ``PdlError`` instead of the reference's
``exit(1)`` (library.cpp:90-93).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .pangene_idata import PangeneIData
from .scores import Scores


def _np_copy(ptr, dtype, n):
    if n == 0:
        return np.zeros(0, dtype)
    buf = (C.c_char * (np.dtype(dtype).itemsize * n)).from_address(C.cast(ptr, C.c_void_p).value)
    return np.frombuffer(buf, dtype=dtype, count=n).copy()


def _gene_arrays(residues, offsets, what="n", where=""):
    """(residues, offsets) as the contiguous uint8 / uint64 arrays the library reads; offsets hold ``what`` + 1 entries
    (``where``: a prefix of the message, such as the query's place in a batch)."""
    res = np.ascontiguousarray(residues, dtype=np.uint8)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    if off.ndim != 1 or len(off) < 1:
        raise _lib.PdlError(_lib.PDL_ERR_ARGUMENT, f"{where}offsets must hold {what} + 1 entries")
    return res, off


def _one_genome(data: PangeneIData, query=None):
    """(residues, offsets) of a ``PangeneIData`` that holds exactly one genome (``query``: its place in a batch, for the message)."""
    residues, offsets, genome_of = data.flatten()
    n_genomes = len(np.unique(genome_of))
    if n_genomes != 1:
        raise ValueError(f"a query holds exactly one genome, {'this data' if query is None else f'query {query}'} holds {n_genomes}")
    return residues, offsets


def _edge_arrays(src, dst, genome_of):
    """An edge list (gene ids ``src`` / ``dst``) and the genes' genome ids as the contiguous int32 / uint32 arrays the library reads."""
    s = np.ascontiguousarray(src, dtype=np.int32)
    d = np.ascontiguousarray(dst, dtype=np.int32)
    g = np.ascontiguousarray(genome_of, dtype=np.uint32)
    if s.ndim != 1 or s.shape != d.shape or g.ndim != 1:
        raise _lib.PdlError(_lib.PDL_ERR_ARGUMENT, "src and dst must be two vectors of one length, genome_of a vector")
    return s, d, g


class PangeneNative:
    def __init__(self, k: int, data: PangeneIData, only_complexity: bool = False, device: int = -1,
                 stream: Optional[int] = None, flags: int = 0):
        residues, offsets, genome_of = data.flatten()
        self._init(k, residues, offsets, genome_of, only_complexity, device, stream, flags)

    @classmethod
    def from_arrays(cls, k, residues, offsets, genome_of, only_complexity=False, device=-1, stream=None, flags=0):
        self = cls.__new__(cls)
        self._init(k, residues, offsets, genome_of, only_complexity, device, stream, flags)
        return self

    @classmethod
    def from_device(cls, k, d_residues: int, d_offsets: int, d_genome_of: int, n_sequences: int, n_residues: int,
                    only_complexity=False, device=-1, stream=None, flags=0, keepalive=None):
        """Device-resident inputs (raw device pointers, e.g. ``tensor.data_ptr()``)."""
        self = cls.__new__(cls)
        self._open(device, stream, flags)
        self.preprocess_device(k, d_residues, d_offsets, d_genome_of, n_sequences, n_residues, only_complexity, keepalive)
        return self

    def preprocess_device(self, k, d_residues: int, d_offsets: int, d_genome_of: int, n_sequences: int,
                          n_residues: int, only_complexity=False, keepalive=None):
        """(Re)run preprocessSequences on this context from device-resident inputs; like the reference's
        entry point it resets all state of the context first (library.cpp:192).  Work buffers are reused."""
        self._keep = keepalive
        self.cost = _lib.PdlCost()
        rc = self._lib.pdl_preprocess_device(self._ctx, d_residues, d_offsets, d_genome_of, n_sequences, n_residues,
                                             int(k), int(only_complexity), C.byref(self.cost))
        self._check(rc)

    @classmethod
    def open(cls, device=-1, stream=None, flags=0) -> "PangeneNative":
        """A context without a dictionary yet (set a genome shard, then preprocess)."""
        self = cls.__new__(cls)
        self._open(device, stream, flags)
        self.cost = _lib.PdlCost()
        return self

    @staticmethod
    def print_complexity(k: int, data: PangeneIData) -> "PangeneNative":
        """PangeneNative.printComplexity (PangeneNative.java:10-12): cost model only."""
        nat = PangeneNative(k, data, only_complexity=True)
        c = nat.cost
        print("------------\nCOMPUTATIONAL COSTS: ")
        print(f"Total cost: {c.total_cost} lookups")
        print(f"Linear ratio: {c.linear_ratio:g}\n------------\n")
        return nat

    # ------------------------------------------------------------------------------------------
    def _open(self, device, stream, flags):
        self._lib = _lib.load()
        cfg = _lib.PdlConfig(device=device, stream=stream or None, flags=flags, reserved=0)
        ctx = self._lib.pdl_create(C.byref(cfg))
        if not ctx:
            raise _lib.PdlError(_lib.PDL_ERR_DEVICE, self._lib.pdl_last_error(None).decode())
        self._ctx = C.c_void_p(ctx)

    def _init(self, k, residues, offsets, genome_of, only_complexity, device, stream, flags):
        self._open(device, stream, flags)
        self.preprocess(k, residues, offsets, genome_of, only_complexity)

    def preprocess(self, k, residues, offsets, genome_of, only_complexity=False):
        """(Re)run preprocessSequences on this context from host arrays."""
        res = np.ascontiguousarray(residues, dtype=np.uint8)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        gen = np.ascontiguousarray(genome_of, dtype=np.uint32)
        self.cost = _lib.PdlCost()
        rc = self._lib.pdl_preprocess(self._ctx, res.ctypes.data, off.ctypes.data, gen.ctypes.data, len(gen), int(k),
                                      int(only_complexity), C.byref(self.cost))
        self._check(rc)

    def ingest_faa(self, path) -> dict:
        """`.faa` -> HBM in one pass (``pdl_ingest_faa``: PangeneIData.readFromFile + calculate_k.py on the way, pinned
        staging buffers, copies overlapped with the parse).  -> sizes, ``k_suggested``, ``genome_names``, host ``offsets`` /
        ``genome_of`` and the device pointers ``preprocess_ingested`` works on."""
        ing = _lib.PdlIngest()
        self._check(self._lib.pdl_ingest_faa(self._ctx, str(path).encode(), C.byref(ing)))
        n = ing.sequences
        return {"file_bytes": ing.file_bytes, "residues": ing.residues, "sequences": n, "genomes": ing.genomes,
                "k_suggested": ing.k_suggested, "parse_ms": ing.parse_ms,
                "offsets": _np_copy(ing.offsets, np.uint64, n + 1), "genome_of": _np_copy(ing.genome_of, np.uint32, n),
                "genome_names": [self._lib.pdl_ingest_genome_name(self._ctx, g).decode("latin-1") for g in range(ing.genomes)],
                "d_residues": ing.d_residues or 0, "d_offsets": ing.d_offsets or 0, "d_genome_of": ing.d_genome_of or 0}

    def preprocess_ingested(self, k, only_complexity=False):
        """preprocessSequences on what ``ingest_faa`` left in HBM."""
        self.cost = _lib.PdlCost()
        self._check(self._lib.pdl_preprocess_ingested(self._ctx, int(k), int(only_complexity), C.byref(self.cost)))

    def _check(self, rc):
        if rc != _lib.PDL_OK:
            raise _lib.PdlError(rc, self._lib.pdl_last_error(self._ctx).decode())

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.pdl_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- reference surface ---------------------------------------------------------------------------
    def generate_scores_part(self, genome: int, multithread: bool = False) -> Scores:
        """PangeneNative.generateScoresPart (PangeneNative.java:17-21); ``multithread`` only selected the
        ignored step_size in the reference (library.cpp:454)."""
        s = _lib.PdlScores()
        self._check(self._lib.pdl_compute_scores(self._ctx, int(genome), C.byref(s)))
        return self._take_scores(s)

    def query_scores(self, residues, offsets) -> Scores:
        """One new genome against this dictionary, without a rebuild (``pdl_query_scores``): the Scores block of genome
        G = ``cost.genomes`` in the union run, with these genes appended as ids N..N+n-1.  ``last_query_info`` then holds
        the call's sizes, "Genome G cost" (``genome_cost``) and device time as a dict."""
        res, off = _gene_arrays(residues, offsets, "n_query")
        s, info = _lib.PdlScores(), _lib.PdlQueryInfo()
        self._check(self._lib.pdl_query_scores(self._ctx, res.ctypes.data if res.size else None, off.ctypes.data,
                                               len(off) - 1, C.byref(s), C.byref(info)))
        self.last_query_info = info.as_dict()
        return self._take_scores(s)

    def query_idata(self, data: PangeneIData) -> Scores:
        """``query_scores`` for the genes of a ``PangeneIData`` that holds exactly one genome."""
        return self.query_scores(*_one_genome(data))

    @staticmethod
    def pack_queries(queries):
        """``[(residues, offsets), ...]`` -> (residues, offsets [n + 1], gene_begin [q + 1]) as ``pdl_query_batch`` takes them:
        the queries' genes one behind the other, ``gene_begin[j]`` the first gene of query j.  Offsets need not start at 0:
        a query's genes are ``residues[offsets[0]:offsets[-1]]``."""
        parts, offs, begin = [], [np.zeros(1, np.uint64)], [0]
        at = 0
        for j, (residues, offsets) in enumerate(queries):
            res, off = _gene_arrays(residues, offsets, where=f"query {j}: ")
            if (np.diff(off.astype(np.int64)) < 0).any() or int(off[-1]) > len(res):
                raise _lib.PdlError(_lib.PDL_ERR_ARGUMENT, f"query {j}: offsets decrease or pass the residues")
            lo, hi = int(off[0]), int(off[-1])
            parts.append(res[lo:hi])
            offs.append((off[1:].astype(np.int64) - lo + at).astype(np.uint64))
            at += hi - lo
            begin.append(begin[-1] + len(off) - 1)
        res = np.concatenate(parts).astype(np.uint8) if parts else np.zeros(0, np.uint8)
        return res, np.concatenate(offs).astype(np.uint64), np.asarray(begin, dtype=np.uint32)

    def query_batch(self, queries) -> list:
        """Many new genomes against this dictionary in one pass, each on its own (``pdl_query_batch``): ``queries`` is a list
        of ``(residues, offsets)``; -> one ``Scores`` per query, the block ``query_scores`` returns for that genome alone.
        ``last_query_batch_info`` then holds ``queries`` (the per-query dicts of ``last_query_info``), ``chunks`` and
        ``device_ms``."""
        queries = list(queries)
        res, off, begin = self.pack_queries(queries)
        q = len(queries)
        blocks = (_lib.PdlScores * max(q, 1))()
        infos = (_lib.PdlQueryInfo * max(q, 1))()
        binfo = _lib.PdlQueryBatchInfo()
        self._check(self._lib.pdl_query_batch(self._ctx, res.ctypes.data if res.size else None, off.ctypes.data, begin.ctypes.data,
                                              len(off) - 1, q, blocks, infos, C.byref(binfo)))
        out = []
        try:
            for j in range(q):
                out.append(self._take_scores(blocks[j]))
        finally:                                         # (a block that was taken is zero: freeing it again does nothing)
            for j in range(len(out), q):
                self._lib.pdl_free_scores(C.byref(blocks[j]))
        self.last_query_batch_info = {"queries": [infos[j].as_dict() for j in range(q)], "chunks": binfo.chunks, "device_ms": binfo.device_ms}
        return out

    def query_batch_idata(self, datas) -> list:
        """``query_batch`` for a list of ``PangeneIData``, each holding exactly one genome."""
        return self.query_batch([_one_genome(data, j) for j, data in enumerate(datas)])

    def append(self, residues, offsets, genome_of=None) -> None:
        """New genomes join this dictionary by a merge, without a rebuild (``pdl_append_genomes``): the genes become ids
        N..N+n-1, all of one new genome G = ``cost.genomes`` (``genome_of`` None) or of the union ids ``genome_of`` (G, G+1, ...
        in first-seen order).  Afterwards the context is the one ``preprocess`` on the union would leave; ``cost`` is the
        union's and ``last_append_info`` holds the call's sizes and device times as a dict.  A refusal leaves everything as
        it was."""
        res, off = _gene_arrays(residues, offsets)
        gen = None
        if genome_of is not None:
            gen = np.ascontiguousarray(genome_of, dtype=np.uint32)
            if gen.shape != (len(off) - 1,):
                raise _lib.PdlError(_lib.PDL_ERR_ARGUMENT, "genome_of must hold one id per gene")
        cost, info = _lib.PdlCost(), _lib.PdlAppendInfo()
        self._check(self._lib.pdl_append_genomes(self._ctx, res.ctypes.data if res.size else None, off.ctypes.data,
                                                 gen.ctypes.data if gen is not None and gen.size else None, len(off) - 1,
                                                 C.byref(cost), C.byref(info)))
        self.cost = cost
        self.last_append_info = info.as_dict()
        self.last_rekey_info = self._rekey_info()

    def append_idata(self, data: PangeneIData) -> None:
        """``append`` for the genes of a ``PangeneIData`` (one genome or several): its genome ids 0, 1, ... become
        G, G+1, ... of this context."""
        residues, offsets, genome_of = data.flatten()
        self.append(residues, offsets, genome_of + np.uint32(self.cost.genomes))

    def remove(self, genomes) -> None:
        """Genomes leave this dictionary by a compaction of the sorted k-mer stream, without a rebuild (``pdl_remove_genomes``):
        ``genomes`` are distinct ids of this context.  Afterwards the context is the one ``preprocess`` on the remaining set
        would leave (genes and genomes renumbered densely in their order); ``cost`` is the remaining set's and
        ``last_remove_info`` holds what left and the device times as a dict.  A refusal leaves everything as it was;
        ``PDL_ERR_UNSUPPORTED`` (the remaining set's alphabet cannot be proved from the keys) asks for a rebuild."""
        ids = np.ascontiguousarray(genomes, dtype=np.uint32).reshape(-1)
        cost, info = _lib.PdlCost(), _lib.PdlRemoveInfo()
        self._check(self._lib.pdl_remove_genomes(self._ctx, ids.ctypes.data if ids.size else None, len(ids), C.byref(cost), C.byref(info)))
        self.cost = cost
        self.last_remove_info = info.as_dict()
        self.last_rekey_info = self._rekey_info()

    def _rekey_info(self) -> dict:
        """What the last append or removal did about the alphabet (``pdl_get_rekey_info``; option ``alphabet_rekey``): letters and
        key bits before and after, keys written again, the pass's device time, and whether the rank table changed at all."""
        info = _lib.PdlRekeyInfo()
        self._check(self._lib.pdl_get_rekey_info(self._ctx, C.byref(info)))
        return info.as_dict()

    @property
    def last_query_rekey_info(self) -> dict:
        """What the last successful ``query_scores`` / ``query_batch`` / ``place_query`` / ``place_batch`` did about letters the base
        lacks (``pdl_get_query_rekey_info``; option ``query_rekey``): queries that brought one, letters and key bits of the base and
        the most a query's union had, records written back into the base's alphabet and that pass's device time."""
        info = _lib.PdlQueryRekeyInfo()
        self._check(self._lib.pdl_get_query_rekey_info(self._ctx, C.byref(info)))
        return info.as_dict()

    @property
    def last_query_join_info(self) -> dict:
        """Which way the rows of the last successful ``query_scores`` / ``query_batch`` / ``place_query`` / ``place_batch`` took
        through the query's join (``pdl_get_query_join_info``): rows joined, rows that might have left the LDS table and rows that
        did, launches of the HBM kernel, the most workgroups one had, and how often its tables were cleared instead of reused."""
        info = _lib.PdlQueryJoinInfo()
        self._check(self._lib.pdl_get_query_join_info(self._ctx, C.byref(info)))
        return info.as_dict()

    def _take_scores(self, s) -> Scores:
        try:
            z, rows, g, n = s.scoresCount, s.rows, s.genomes, s.sequences
            out = Scores(
                scoresCount=z,
                scores=_np_copy(s.scores, np.float32, z), percs=_np_copy(s.percs, np.float32, z),
                tr_percs=_np_copy(s.tr_percs, np.float32, z),
                row=_np_copy(s.row, np.int32, z), column=_np_copy(s.column, np.int32, z),
                first_seq_genome=_np_copy(s.first_seq_genome, np.int32, z),
                second_seq_genome=_np_copy(s.second_seq_genome, np.int32, z),
                max_genome_score=_np_copy(s.max_genome_score, np.float32, rows * g).reshape(rows, g),
                max_genome_score_col=_np_copy(s.max_genome_score_col, np.float32, n),
                scoresMaxMappings=_np_copy(s.scoresMaxMappings, np.int32, n))
        finally:
            self._lib.pdl_free_scores(C.byref(s))
        return out

    def generate_edges_part(self, genome: int):
        """The best-hit filter of the Java host (Pangenes.java:98-176) for one genome task, run on the device: -> (src, dst,
        score) of the edges the task adds to the network, in the host's insertion order."""
        e = _lib.PdlEdges()
        self._check(self._lib.pdl_compute_edges(self._ctx, int(genome), C.byref(e)))
        try:
            n = e.count
            return (_np_copy(e.src, np.int32, n).astype(np.int64), _np_copy(e.dst, np.int32, n).astype(np.int64), _np_copy(e.score, np.float32, n))
        finally:
            self._lib.pdl_free_edges(C.byref(e))

    def generate_families(self) -> dict:
        """K-fam over this context's own edges, where they lie in HBM (``pdl_compute_families``): the network's connected
        components and their collision flags -> the fields of ``pdl_families`` as a dict (counts as ints, arrays as numpy).
        ``netclu.families_from_components`` makes the gene families of it.  ``last_families_info`` holds the counts and the
        device time."""
        f = _lib.PdlFamilies()
        self._check(self._lib.pdl_compute_families(self._ctx, C.byref(f)))
        return self._take_families(f)

    def families_of_edges(self, src, dst, genome_of) -> dict:
        """The same kernels over a caller's edge list (``pdl_families_of_edges``): gene ids ``src`` / ``dst``, one genome id per
        gene — a network gathered from genome batches or from several ranks.  Needs no preprocess and leaves the context's own
        state alone."""
        s, d, g = _edge_arrays(src, dst, genome_of)
        f = _lib.PdlFamilies()
        self._check(self._lib.pdl_families_of_edges(self._ctx, s.ctypes.data if s.size else None, d.ctypes.data if d.size else None, len(s),
                                                    g.ctypes.data if g.size else None, len(g), C.byref(f)))
        return self._take_families(f)

    def _take_families(self, f) -> dict:
        try:
            n, nodes, fams = f.sequences, f.nodes, f.families
            out = {"sequences": n, "nodes": nodes, "families": fams, "colliding": f.colliding,
                   "component_of": _np_copy(f.component_of, np.uint32, n), "is_node": _np_copy(f.is_node, np.uint8, n),
                   "family_off": _np_copy(f.family_off, np.uint32, fams + 1), "family_genes": _np_copy(f.family_genes, np.uint32, nodes),
                   "collides": _np_copy(f.collides, np.uint8, fams)}
            self.last_families_info = {"sequences": n, "nodes": nodes, "families": fams, "colliding": f.colliding, "device_ms": f.device_ms}
        finally:
            self._lib.pdl_free_families(C.byref(f))
        return out

    def split_packed(self, node_off, adj_off, adj) -> list:
        """``pdl_split_first_level`` on arrays as ``netclu.pack_graphs`` makes them -> per graph the removed edges, in removal
        order, as (u, v) pairs of LOCAL indices.  ``last_split_info`` holds graphs, nodes, edges, removals, rounds, chunks and the
        device time of the call."""
        no = np.ascontiguousarray(node_off, dtype=np.uint64)
        ao = np.ascontiguousarray(adj_off, dtype=np.uint64)
        ad = np.ascontiguousarray(adj, dtype=np.uint32)
        s = _lib.PdlSplit()
        self._check(self._lib.pdl_split_first_level(self._ctx, max(len(no) - 1, 0), no.ctypes.data if no.size else None,
                                                    ao.ctypes.data if ao.size else None, ad.ctypes.data if ad.size else None, C.byref(s)))
        try:
            off = _np_copy(s.removed_off, np.uint64, s.graphs + 1)
            u, v = _np_copy(s.removed_u, np.uint32, s.removals).tolist(), _np_copy(s.removed_v, np.uint32, s.removals).tolist()
            self.last_split_info = {"graphs": s.graphs, "nodes": s.nodes, "edges": s.edges, "removals": s.removals, "rounds": s.rounds,
                                    "chunks": s.chunks, "device_ms": s.device_ms}
        finally:
            self._lib.pdl_free_split(C.byref(s))
        return [list(zip(u[int(off[j]):int(off[j + 1])], v[int(off[j]):int(off[j + 1])])) for j in range(len(off) - 1)]

    def split_first_level(self, graphs) -> list:
        """The first level of Girvan-Newman on every graph of ``graphs`` (ordered adjacencies, ``g = rebuilt(rebuilt(view))`` of
        ``netclu.girvan_newman_first_level``) in one call on the device -> per graph the removed edges in removal order, named by
        their nodes as ``netclu.edge_list`` names them.  The splitter ``netclu.split_all_until_clean`` takes.  Needs no
        preprocess and leaves the context's own state alone."""
        from . import netclu
        if not graphs:
            return []
        node_off, adj_off, adj, keys = netclu.pack_graphs(graphs)
        return [[(ks[u], ks[v]) for u, v in rem] for ks, rem in zip(keys, self.split_packed(node_off, adj_off, adj))]

    def family_profile(self, family_of, genome_of, n_genomes: int) -> dict:
        """The pan-genome profile of a labelling (``pdl_family_profile``): a family is the set of genes with equal
        ``family_of`` (any label below the gene count; a gene in no family carries a label of its own) -> the fields of
        ``pdl_profile`` as a dict: counts as ints, arrays as numpy (``spread_by_genome`` as a (G + 1, G) table).  Needs no
        preprocess and leaves the context's own state alone.  ``last_profile_info`` holds families, incidences and the device
        time of the call."""
        fam = np.ascontiguousarray(family_of, dtype=np.uint32)
        gen = np.ascontiguousarray(genome_of, dtype=np.uint32)
        if fam.shape != gen.shape or fam.ndim != 1:
            raise ValueError("family_of and genome_of: one label and one genome id per gene")
        p = _lib.PdlProfile()
        self._check(self._lib.pdl_family_profile(self._ctx, fam.ctypes.data if fam.size else None, gen.ctypes.data if gen.size else None,
                                                 len(fam), int(n_genomes), C.byref(p)))
        try:
            F, Z, G = p.families, p.incidences, p.n_genomes
            out = {n: getattr(p, n) for n in ("n_sequences", "n_genomes", "families", "incidences", "max_size", "core", "single_copy_core",
                                              "unique", "accessory")}
            for name, count in (("label", F), ("size", F), ("spread", F), ("genome_off", F + 1), ("genomes", Z), ("copies", Z),
                                ("size_hist", p.max_size + 1), ("spread_hist", G + 1), ("spread_by_genome", (G + 1) * G),
                                ("genome_genes", G), ("genome_core", G), ("genome_accessory", G), ("genome_unique", G)):
                out[name] = _np_copy(getattr(p, name), np.uint32, count)
            out["spread_by_genome"] = out["spread_by_genome"].reshape(G + 1, G)
            self.last_profile_info = {"families": F, "incidences": Z, "device_ms": p.device_ms}
        finally:
            self._lib.pdl_free_profile(C.byref(p))
        return out

    def pan_curves(self, profile: dict, orders) -> dict:
        """Pan and core accumulation curves of a profile (``family_profile``'s dict) over genome orders (``pdl_pan_curves``):
        ``orders`` is (n_orders, G), every row a permutation of 0..G-1 (``pangenome.random_orders`` makes them on the host) ->
        {"pan", "core"}: (n_orders, G) exact counts, pan[o, i] = families with a gene in at least one of the first i + 1 genomes
        of order o, core[o, i] = in every one of them.  ``last_curves_info`` holds families, incidences, orders and the device
        time of the call."""
        o = np.ascontiguousarray(orders, dtype=np.uint32)
        G = int(profile["n_genomes"])
        if o.ndim != 2 or o.shape[1] != G:
            raise ValueError(f"orders: (n_orders, {G})")
        keep = {n: np.ascontiguousarray(profile[n], dtype=np.uint32) for n in ("spread", "genome_off", "genomes")}
        p = _lib.PdlProfile(n_genomes=G, families=int(profile["families"]), incidences=int(profile["incidences"]), core=int(profile["core"]))
        for n, a in keep.items():
            setattr(p, n, a.ctypes.data_as(_lib._pu32))
        cv = _lib.PdlCurves()
        self._check(self._lib.pdl_pan_curves(self._ctx, C.byref(p), o.ctypes.data if o.size else None, o.shape[0], C.byref(cv)))
        try:
            cells = cv.n_orders * cv.n_genomes
            out = {"pan": _np_copy(cv.pan, np.uint32, cells).reshape(cv.n_orders, cv.n_genomes),
                   "core": _np_copy(cv.core, np.uint32, cells).reshape(cv.n_orders, cv.n_genomes)}
            self.last_curves_info = {"families": cv.families, "incidences": cv.incidences, "orders": cv.n_orders, "device_ms": cv.device_ms}
        finally:
            self._lib.pdl_free_curves(C.byref(cv))
        return out

    def genome_matrix(self, profile: dict) -> dict:
        """The genome-by-genome shared-family matrices of a profile (``family_profile``'s dict; ``pdl_genome_matrix``) ->
        {"shared", "shared_copies"}: (G, G) uint32, exact — shared[g, h] = families with a gene in g and in h, shared_copies[g, h]
        = the sum over the families of min(copies in g, copies in h) — and the scalars n_genomes, families, incidences, levels,
        slabs, splits and device_ms, which ``last_matrix_info`` holds as well.  ``pangenome.jaccard_distance`` and
        ``pair_pan_core`` take the matrices.  Needs no preprocess and leaves the context's own state alone."""
        G = int(profile["n_genomes"])
        keep = {n: np.ascontiguousarray(profile[n], dtype=np.uint32) for n in ("size", "spread", "genome_off", "genomes", "copies")}
        p = _lib.PdlProfile(n_sequences=int(profile["n_sequences"]), n_genomes=G, families=int(profile["families"]),
                            incidences=int(profile["incidences"]), core=int(profile["core"]))
        for n, a in keep.items():
            setattr(p, n, a.ctypes.data_as(_lib._pu32))
        m = _lib.PdlGenomeMatrix()
        self._check(self._lib.pdl_genome_matrix(self._ctx, C.byref(p), C.byref(m)))
        try:
            info = {n: getattr(m, n) for n in ("n_genomes", "families", "incidences", "levels", "slabs", "splits", "device_ms")}
            out = {"shared": _np_copy(m.shared, np.uint32, G * G).reshape(G, G),
                   "shared_copies": _np_copy(m.shared_copies, np.uint32, G * G).reshape(G, G), **info}
            self.last_matrix_info = info
        finally:
            self._lib.pdl_free_genome_matrix(C.byref(m))
        return out

    def place_query(self, residues, offsets) -> dict:
        """One new genome placed into this context's gene families, without a commit (``pdl_place_query``): the query's edges
        (``src``, ``dst``, ``score`` in the host's insertion order, ``edges_phase1`` of them phase 1) and, per query gene and per
        group the query touches, the fields of ``pdl_placement`` as a dict (counts as ints, arrays as numpy).  The context is
        only read.  ``last_place_info`` holds the counts, the device time and the query's own ``pdl_query_info`` (``query``)."""
        res, off = _gene_arrays(residues, offsets, "n_query")
        p, info = _lib.PdlPlacement(), _lib.PdlQueryInfo()
        self._check(self._lib.pdl_place_query(self._ctx, res.ctypes.data if res.size else None, off.ctypes.data, len(off) - 1,
                                              C.byref(p), C.byref(info)))
        return self._take_placement(p, True, info.as_dict())

    def place_idata(self, data: PangeneIData) -> dict:
        """``place_query`` for the genes of a ``PangeneIData`` that holds exactly one genome."""
        return self.place_query(*_one_genome(data))

    def place_batch(self, queries) -> list:
        """Many new genomes placed into this context's gene families in one pass, each on its own (``pdl_place_batch``):
        ``queries`` is a list of ``(residues, offsets)``; -> one dict per query, the one ``place_query`` returns for that
        genome alone (ids are that query's own union ids).  ``last_place_batch_info`` then holds ``queries`` (per query: the
        counts, ``edges``, ``device_ms`` and its ``pdl_query_info`` as ``query``), ``chunks`` and ``device_ms``."""
        queries = list(queries)
        res, off, begin = self.pack_queries(queries)
        q = len(queries)
        pls = (_lib.PdlPlacement * max(q, 1))()
        infos = (_lib.PdlQueryInfo * max(q, 1))()
        binfo = _lib.PdlPlaceBatchInfo()
        self._check(self._lib.pdl_place_batch(self._ctx, res.ctypes.data if res.size else None, off.ctypes.data, begin.ctypes.data,
                                              len(off) - 1, q, pls, infos, C.byref(binfo)))
        out, per_query = self._take_placements(pls, q, True, [infos[j].as_dict() for j in range(q)])
        self.last_place_batch_info = {"queries": per_query, "chunks": binfo.chunks, "device_ms": binfo.device_ms}
        return out

    def place_batch_idata(self, datas) -> list:
        """``place_batch`` for a list of ``PangeneIData``, each holding exactly one genome."""
        return self.place_batch([_one_genome(data, j) for j, data in enumerate(datas)])

    @staticmethod
    def pack_edge_lists(edge_lists):
        """``[(src, dst), ...]`` -> (src, dst, edge_begin [q + 1]) as ``pdl_placement_batch_of_edges`` takes them: the lists laid
        end to end, ``edge_begin[j]`` the first edge of list j."""
        ss, dd, begin = [], [], [0]
        for j, (src, dst) in enumerate(edge_lists):
            s = np.ascontiguousarray(src, dtype=np.int32)
            d = np.ascontiguousarray(dst, dtype=np.int32)
            if s.ndim != 1 or s.shape != d.shape:
                raise _lib.PdlError(_lib.PDL_ERR_ARGUMENT, f"query {j}: src and dst must be two vectors of one length")
            ss.append(s); dd.append(d); begin.append(begin[-1] + len(s))
        cat = lambda parts: np.ascontiguousarray(np.concatenate(parts), dtype=np.int32) if parts else np.zeros(0, np.int32)
        return cat(ss), cat(dd), np.asarray(begin, dtype=np.uint64)

    def placement_batch_of_edges(self, base: dict, genome_of, n_query, edge_lists) -> list:
        """The batch form of ``placement_of_edges`` (``pdl_placement_batch_of_edges``): one base, ``n_query[j]`` query genes
        and the edge list ``edge_lists[j] = (src, dst)`` in query j's own union ids per query; every list is checked on the
        device against its own id range.  -> one dict per query, as ``placement_of_edges`` on that list alone."""
        s, d, begin = self.pack_edge_lists(edge_lists)
        nq = np.ascontiguousarray(n_query, dtype=np.uint32).reshape(-1)
        if len(nq) != len(begin) - 1:
            raise _lib.PdlError(_lib.PDL_ERR_ARGUMENT, "n_query must hold one count per edge list")
        fam, g, keep = self._base_families(base, genome_of)
        q = len(nq)
        pls = (_lib.PdlPlacement * max(q, 1))()
        self._check(self._lib.pdl_placement_batch_of_edges(self._ctx, C.byref(fam), g.ctypes.data if g.size else None, q,
                                                           nq.ctypes.data if nq.size else None, begin.ctypes.data,
                                                           s.ctypes.data if s.size else None, d.ctypes.data if d.size else None, pls))
        del keep
        return self._take_placements(pls, q, False, [None] * q)[0]

    def _take_placements(self, pls, q, with_edges, query_infos):
        """The q placements of a batch as dicts (each is freed as it is taken; the rest after a failure) and their infos."""
        out, infos = [], []
        try:
            for j in range(q):
                out.append(self._take_placement(pls[j], with_edges, query_infos[j]))
                infos.append(self.last_place_info)
        finally:                                         # (a placement that was taken is zero: freeing it again does nothing)
            for j in range(len(out), q):
                self._lib.pdl_free_placement(C.byref(pls[j]))
        return out, infos

    @staticmethod
    def _base_families(base: dict, genome_of):
        """A families dict and the genes' genomes as the ``pdl_families`` a placement of a caller's edges reads (and the arrays
        it points into, to be kept alive over the call)."""
        g = np.ascontiguousarray(genome_of, dtype=np.uint32)
        if g.ndim != 1:
            raise _lib.PdlError(_lib.PDL_ERR_ARGUMENT, "genome_of must be a vector")
        keep = {f: np.ascontiguousarray(base[f], dtype=t) for f, t in (("component_of", np.uint32), ("is_node", np.uint8), ("family_off", np.uint32),
                                                                        ("family_genes", np.uint32), ("collides", np.uint8))}
        if len(keep["component_of"]) != len(g) or len(keep["is_node"]) != len(g) or len(keep["family_off"]) != len(keep["collides"]) + 1:
            raise _lib.PdlError(_lib.PDL_ERR_ARGUMENT, "the base families do not describe len(genome_of) genes")
        fam = _lib.PdlFamilies(sequences=len(g), nodes=len(keep["family_genes"]), families=len(keep["collides"]), colliding=int(keep["collides"].sum()))
        for f, a in keep.items():
            setattr(fam, f, a.ctypes.data_as(dict(_lib.PdlFamilies._fields_)[f]))
        return fam, g, keep

    def placement_of_edges(self, base: dict, genome_of, n_query: int, src, dst) -> dict:
        """The same kernels over a caller's query edge list in union ids (``pdl_placement_of_edges``): ``base`` is the dict
        ``generate_families`` / ``families_of_edges`` returned for the N base genes, ``genome_of`` their genomes; the query is
        ``n_query`` genes N..N+n_query-1 of one further genome.  Needs no preprocess and leaves the context's own state alone."""
        s, d, g = _edge_arrays(src, dst, genome_of)
        fam, g, keep = self._base_families(base, g)
        p = _lib.PdlPlacement()
        self._check(self._lib.pdl_placement_of_edges(self._ctx, C.byref(fam), g.ctypes.data if g.size else None, int(n_query),
                                                     s.ctypes.data if s.size else None, d.ctypes.data if d.size else None, len(s), C.byref(p)))
        return self._take_placement(p, False, None)

    def _take_placement(self, p, with_edges, query_info) -> dict:
        try:
            n, groups, e = p.n_query, p.groups, p.edges
            counts = {f: int(getattr(p, f)) for f in ("sequences", "n_query", "genomes", "edges_phase1", "groups", "novel", "joined", "bridging",
                                                       "colliding", "unplaced")}
            q_off = _np_copy(p.group_query_off, np.uint32, groups + 1)
            b_off = _np_copy(p.group_base_off, np.uint32, groups + 1)
            out = dict(counts)
            out.update({"family_of": _np_copy(p.family_of, np.uint32, n), "is_node": _np_copy(p.is_node, np.uint8, n),
                        "group_label": _np_copy(p.group_label, np.uint32, groups), "group_query_off": q_off,
                        "group_query": _np_copy(p.group_query, np.uint32, int(q_off[-1])), "group_base_off": b_off,
                        "group_base": _np_copy(p.group_base, np.uint32, int(b_off[-1])), "group_collides": _np_copy(p.group_collides, np.uint8, groups)})
            if with_edges:
                out.update({"src": _np_copy(p.src, np.int32, e).astype(np.int64), "dst": _np_copy(p.dst, np.int32, e).astype(np.int64),
                            "score": _np_copy(p.score, np.float32, e)})
            self.last_place_info = dict(counts, edges=int(e), device_ms=float(p.device_ms), query=query_info)
        finally:
            self._lib.pdl_free_placement(C.byref(p))
        return out

    # -- beyond the reference surface (device-resident batch, sharding, introspection) ------------------
    def score_all(self) -> None:
        self._check(self._lib.pdl_score_all(self._ctx))

    def set_option(self, name: str, value: int) -> None:
        """Tuning / test switch of this context (``pdl_set_option``; the library reads no environment variable)."""
        self._check(self._lib.pdl_set_option(self._ctx, name.encode(), int(value)))

    # -- multi-GPU passes (one context per GPU; pandelos_amd.distributed moves the bytes in between) ------------
    def dist_preprocess_begin(self, k, d_residues: int, d_offsets: int, d_genome_of: int, n_sequences: int,
                              n_residues: int, world: int, rank: int, keepalive=None):
        """-> (device pointer, records, k-mers) of this rank's run of the dictionary; ``self.run_weights`` = every genome's
        lookups above the diagonal inside the run (int64 [G])."""
        self._keep = keepalive
        sl = _lib.PdlDistSlice()
        self._check(self._lib.pdl_dist_preprocess_begin(self._ctx, d_residues, d_offsets, d_genome_of, n_sequences, n_residues,
                                                        int(k), int(world), int(rank), C.byref(sl)))
        self.run_weights = np.ctypeslib.as_array(sl.genome_weights, shape=(sl.genomes,)).astype(np.int64) if sl.genomes else np.zeros(0, np.int64)
        self.run_costs = np.ctypeslib.as_array(sl.genome_costs, shape=(sl.genomes,)).astype(np.int64) if sl.genomes else np.zeros(0, np.int64)
        return sl.d_postings or 0, int(sl.records), int(sl.kmers)

    def dist_preprocess_ranges(self, run_records, genome_weights, genome_costs):
        """The range tuples of this rank's run, filed by the rank that owns the gene (between begin and finish; the runs are
        gathered AFTER it).  ``run_records`` [world]; ``genome_weights`` / ``genome_costs`` [G]: the ranks' ``run_weights`` /
        ``run_costs`` summed.  -> None when this build cannot go that way (every rank gets the same answer: use
        ``dist_preprocess_finish``), else (device pointer of the keys, of the packed ranges, tuples per destination rank [world],
        counters [3] of this run: shared records, groups, repeat statistic)."""
        rr = np.ascontiguousarray(run_records, dtype=np.uint64)
        w = np.ascontiguousarray(genome_weights, dtype=np.uint64)
        cs = np.ascontiguousarray(genome_costs, dtype=np.uint64)
        out = _lib.PdlDistRanges()
        self._check(self._lib.pdl_dist_preprocess_ranges(self._ctx, rr.ctypes.data, w.ctypes.data, cs.ctypes.data, C.byref(out)))
        if not out.available:
            return None
        counts = np.array([out.counts[d] for d in range(len(rr))], dtype=np.int64)
        assert int(counts.sum()) == out.total
        return out.d_keys or 0, out.d_ranges or 0, counts, np.array([out.shared_records, out.groups, out.repeat_sample], dtype=np.int64)

    def dist_preprocess_finish_ranges(self, d_postings_all: int, total_records: int, d_keys: int, d_ranges: int, n_tuples: int,
                                      counter_sums, keepalive=None) -> None:
        """Adopts the gathered dictionary and sorts the received tuples (source-rank major) by gene.  ``counter_sums`` [3]: the
        ranks' counters summed.  The three device arrays must stay alive until the next preprocess (``keepalive``)."""
        self._keep_dict = keepalive
        self.cost = _lib.PdlCost()
        sums = np.ascontiguousarray(counter_sums, dtype=np.uint64)
        self._check(self._lib.pdl_dist_preprocess_finish_ranges(self._ctx, d_postings_all, int(total_records), d_keys, d_ranges, int(n_tuples),
                                                                sums.ctypes.data, C.byref(self.cost)))

    def dist_preprocess_finish(self, d_postings_all: int, total_records: int, genome_weights=None, keepalive=None) -> None:
        """``genome_weights``: the ranks' ``run_weights`` summed (identical on every rank); None lets the library compute them."""
        self._keep_dict = keepalive
        self.cost = _lib.PdlCost()
        w = None
        if genome_weights is not None:
            w = np.ascontiguousarray(genome_weights, dtype=np.uint64)
        self._check(self._lib.pdl_dist_preprocess_finish(self._ctx, d_postings_all, int(total_records),
                                                         w.ctypes.data if w is not None else None, C.byref(self.cost)))

    def dist_genome_owner(self) -> np.ndarray:
        out = np.zeros(self.cost.genomes, np.uint32)
        self._check(self._lib.pdl_dist_genome_owner(self._ctx, out.ctypes.data))
        return out

    def dist_score_begin(self, world: int):
        """-> (device pointer of the outbox, cells per destination rank [world])."""
        ob = _lib.PdlDistOutbox()
        self._check(self._lib.pdl_dist_score_begin(self._ctx, C.byref(ob)))
        counts = np.array([ob.counts[d] for d in range(world)], dtype=np.int64)
        assert int(counts.sum()) == ob.total
        return ob.d_cells or 0, counts

    def dist_score_finish(self, d_inbox: int, n_inbox: int, keepalive=None) -> None:
        self._keep_inbox = keepalive
        self._check(self._lib.pdl_dist_score_finish(self._ctx, d_inbox, int(n_inbox)))

    def copy_device(self, d_dst: int, d_src: int, nbytes: int) -> None:
        self._check(self._lib.pdl_copy_device(self._ctx, d_dst, d_src, int(nbytes)))

    def set_genome_shard(self, genomes: Sequence[int]) -> None:
        g = np.ascontiguousarray(genomes, dtype=np.uint32)
        self._check(self._lib.pdl_set_genome_shard(self._ctx, g.ctypes.data, len(g)))

    def scores_in_batches(self, k, residues, offsets, genome_of, genomes_per_batch: int, low_memory: bool = True):
        """Score a set a batch of genomes at a time and yield ``(genome, Scores)`` for every genome in ascending order — for sets
        whose maxima, staging and cells do not fit the device together (the reference's own granularity: one task per genome
        with private scratch, Pangenes.java:60-66, library.cpp:417-428).  The dictionary is built once, with the first batch as
        the genome shard; every further batch costs the two passes over the postings that form its genes' range lists
        (``pdl_set_genome_shard`` on an existing dictionary).  Batches are scored without the row/column symmetry of the
        whole-set pass (a cell's mirror belongs to another batch), i.e. with the reference's full lookup count."""
        gen = np.ascontiguousarray(genome_of, dtype=np.uint32)
        n_genomes = int(gen.max()) + 1 if len(gen) else 0
        if low_memory:
            self.set_option("low_memory", 1)
        for g0 in range(0, n_genomes, max(1, int(genomes_per_batch))):
            batch = list(range(g0, min(n_genomes, g0 + max(1, int(genomes_per_batch)))))
            self.set_genome_shard(batch)
            if g0 == 0:
                self.preprocess(k, residues, offsets, gen)
            for g in batch:
                yield g, self.generate_scores_part(g)

    def genome_cost(self, genome: int) -> int:
        v = C.c_uint64()
        self._check(self._lib.pdl_genome_cost(self._ctx, genome, C.byref(v)))
        return v.value

    def sequence_costs(self):
        n = self.cost.sequences
        cost = np.zeros(n, np.uint64)
        kl = np.zeros(n, np.uint32)
        self._check(self._lib.pdl_sequence_costs(self._ctx, cost.ctypes.data, kl.ctypes.data))
        return cost, kl

    def scores_counts(self) -> np.ndarray:
        out = np.zeros(self.cost.genomes, np.uint32)
        self._check(self._lib.pdl_scores_counts(self._ctx, out.ctypes.data))
        return out

    def dictionary(self):
        u = self.cost.dictionary_records
        ranks, seqs, counts = np.zeros(u, np.uint64), np.zeros(u, np.uint32), np.zeros(u, np.uint32)
        self._check(self._lib.pdl_get_dictionary(self._ctx, ranks.ctypes.data, seqs.ctypes.data, counts.ctypes.data))
        return ranks, seqs, counts

    def rank_table(self):
        tab = np.zeros(256, np.uint8)
        lm = C.c_uint64()
        self._check(self._lib.pdl_get_rank_table(self._ctx, tab.ctypes.data, C.byref(lm)))
        return tab, lm.value

    def timings(self) -> dict:
        return self.timings_struct().as_dict()

    def timings_struct(self):
        """pdl_timings as the ctypes structure (no dictionary is built: for callers inside a timed loop)."""
        t = _lib.PdlTimings()
        self._check(self._lib.pdl_get_timings(self._ctx, C.byref(t)))
        return t
