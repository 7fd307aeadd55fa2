"""pdl_place_batch / pdl_placement_batch_of_edges without a GPU: the header's declarations, the libraries' export tables, the
gene_begin / edge_begin packing of the bindings against a stub library, and the command's label refusals."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def _write(path, recs):
    path.write_bytes(b"".join(b"%s\t%s\tp %s\n%s\n" % (g, n, n, s) for g, n, s in recs))
    return path


def test_the_header_declares_both_functions():
    header = (ROOT / "include" / "pandelos_amd.h").read_text()
    squeeze = lambda s: re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", s, flags=re.S)).strip()
    m = re.search(r"PDL_API\s+int\s+pdl_place_batch\s*\((.*?)\)\s*;", header, flags=re.S)
    assert m, "pdl_place_batch is not declared"
    assert squeeze(m.group(1)) == ("pdl_ctx *, const uint8_t *residues, const uint64_t *offsets , const uint32_t *gene_begin , "
                                   "uint32_t n, uint32_t n_queries, pdl_placement *out , pdl_query_info *info , pdl_place_batch_info *binfo")
    m = re.search(r"PDL_API\s+int\s+pdl_placement_batch_of_edges\s*\((.*?)\)\s*;", header, flags=re.S)
    assert m, "pdl_placement_batch_of_edges is not declared"
    assert squeeze(m.group(1)) == ("pdl_ctx *, const pdl_families *base, const uint32_t *genome_of , uint32_t n_queries, const uint32_t *n_query , "
                                   "const uint64_t *edge_begin , const int32_t *src, const int32_t *dst, pdl_placement *out")
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*pdl_place_batch_info\s*;", header)
    assert m and squeeze(m.group(1)) == "uint32_t queries, chunks; float device_ms;"
    from pandelos_amd import _lib
    assert "pdl_place_batch" in _lib.EXPORTS and "pdl_placement_batch_of_edges" in _lib.EXPORTS
    assert [(n, C.sizeof(t)) for n, t in _lib.PdlPlaceBatchInfo._fields_] == [("queries", 4), ("chunks", 4), ("device_ms", 4)]


@pytest.mark.parametrize("lib", ["libpandelos_amd.so", "libnative.so"])
@pytest.mark.parametrize("symbol", ["pdl_place_batch", "pdl_placement_batch_of_edges"])
def test_libraries_export_the_symbols(lib, symbol):
    from pandelos_amd import _lib
    assert hasattr(C.CDLL(str(_lib.LIB_DIR / lib)), symbol)


class _StubLib:
    """Stands in for libpandelos_amd.so: records what the two entry points were given, answers with placements of j + 1 unplaced genes."""

    def __init__(self):
        self.calls, self.freed, self.alive = [], 0, []

    @staticmethod
    def _np(addr, ct, count):
        return np.ctypeslib.as_array(C.cast(addr, C.POINTER(ct)), shape=(count,)).copy() if count and addr else np.zeros(0, ct)

    def _answer(self, out, n_queries, sequences):
        for j in range(n_queries):
            n = j + 1
            keep = [np.arange(sequences, sequences + n, dtype=np.uint32), np.zeros(n, np.uint8), np.zeros(1, np.uint32), np.zeros(1, np.uint32)]
            self.alive.append(keep)
            out[j].sequences, out[j].n_query, out[j].genomes, out[j].unplaced, out[j].device_ms = sequences, n, 3, n, 0.25
            out[j].family_of = keep[0].ctypes.data_as(C.POINTER(C.c_uint32))
            out[j].is_node = keep[1].ctypes.data_as(C.POINTER(C.c_uint8))
            out[j].group_query_off = keep[2].ctypes.data_as(C.POINTER(C.c_uint32))
            out[j].group_base_off = keep[3].ctypes.data_as(C.POINTER(C.c_uint32))

    def pdl_place_batch(self, ctx, residues, offsets, gene_begin, n, n_queries, out, info, binfo):
        off = self._np(offsets, C.c_uint64, n + 1)
        self.calls.append({"residues": self._np(residues, C.c_uint8, int(off[-1])), "offsets": off,
                           "gene_begin": self._np(gene_begin, C.c_uint32, n_queries + 1), "n": n, "n_queries": n_queries})
        self._answer(out, n_queries, 10)
        for j in range(n_queries):
            info[j].genome_cost = 100 + j
        b = binfo._obj                                                # (what C.byref wraps)
        b.queries, b.chunks, b.device_ms = n_queries, 2, 1.5
        return 0

    def pdl_placement_batch_of_edges(self, ctx, base, genome_of, n_queries, n_query, edge_begin, src, dst, out):
        begin = self._np(edge_begin, C.c_uint64, n_queries + 1)
        fam = base._obj
        self.calls.append({"sequences": fam.sequences, "families": fam.families, "nodes": fam.nodes,
                           "component_of": self._np(fam.component_of, C.c_uint32, fam.sequences), "genome_of": self._np(genome_of, C.c_uint32, fam.sequences),
                           "n_queries": n_queries, "n_query": self._np(n_query, C.c_uint32, n_queries), "edge_begin": begin,
                           "src": self._np(src, C.c_int32, int(begin[-1])), "dst": self._np(dst, C.c_int32, int(begin[-1]))})
        self._answer(out, n_queries, fam.sequences)
        return 0

    def pdl_free_placement(self, p):
        self.freed += 1

    def pdl_last_error(self, ctx):
        return b"stub"


def _stubbed():
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.__new__(PangeneNative)
    nat._lib, nat._ctx = _StubLib(), None
    return nat


def test_place_batch_packs_gene_begin_for_the_library():
    from pandelos_amd.pangene_idata import PangeneIData
    nat = _stubbed()
    q0 = (np.frombuffer(b"ACDEFGHIK", np.uint8), np.array([0, 4, 9], np.uint64))
    q1 = (np.frombuffer(b"xxLMNPQyy", np.uint8), np.array([2, 7], np.uint64))                # offsets that do not start at 0
    q2 = (np.frombuffer(b"RSTVW", np.uint8), [0, 0, 2, 5])                                    # an empty gene, a plain list
    pls = nat.place_batch([q0, q1, q2])
    call, = nat._lib.calls
    assert call["n"] == 6 and call["n_queries"] == 3
    assert call["gene_begin"].tolist() == [0, 2, 3, 6] and call["gene_begin"].dtype == np.uint32
    assert call["offsets"].tolist() == [0, 4, 9, 14, 14, 16, 19]
    assert call["residues"].tobytes() == b"ACDEFGHIKLMNPQRSTVW"
    assert [pl["n_query"] for pl in pls] == [1, 2, 3] and [pl["family_of"].tolist() for pl in pls] == [[10], [10, 11], [10, 11, 12]]
    assert all(len(pl["src"]) == 0 and pl["src"].dtype == np.int64 and pl["score"].dtype == np.float32 for pl in pls)
    assert nat._lib.freed == 3                                                                # every placement goes back to the library
    info = nat.last_place_batch_info
    assert info["chunks"] == 2 and info["device_ms"] == 1.5
    assert [q["query"]["genome_cost"] for q in info["queries"]] == [100, 101, 102]
    assert [q["unplaced"] for q in info["queries"]] == [1, 2, 3] and all(q["device_ms"] == 0.25 and q["edges"] == 0 for q in info["queries"])
    with pytest.raises(ValueError, match="query 1 holds 2"):
        nat.place_batch_idata([PangeneIData.from_arrays(q0[0], q0[1], [0, 0]), PangeneIData.from_arrays(q0[0], q0[1], [0, 1])])
    nat._ctx = None


def test_placement_batch_of_edges_packs_edge_begin_for_the_library():
    from pandelos_amd import _lib
    from pandelos_amd.pangene_native import PangeneNative
    nat = _stubbed()
    base = {"component_of": [0, 0, 2, 3], "is_node": [1, 1, 0, 0], "family_off": [0, 2], "family_genes": [0, 1], "collides": [0]}
    genome_of = [0, 1, 0, 1]
    lists = [([4, 5], [0, 4]), ([], []), (np.array([4], np.int64), np.array([2], np.int64))]
    pls = nat.placement_batch_of_edges(base, genome_of, [2, 1, 3], lists)
    call, = nat._lib.calls
    assert call["n_queries"] == 3 and call["n_query"].tolist() == [2, 1, 3] and call["n_query"].dtype == np.uint32
    assert call["edge_begin"].tolist() == [0, 2, 2, 3] and call["edge_begin"].dtype == np.uint64
    assert call["src"].tolist() == [4, 5, 4] and call["dst"].tolist() == [0, 4, 2] and call["src"].dtype == np.int32
    assert (call["sequences"], call["families"], call["nodes"]) == (4, 1, 2)
    assert call["component_of"].tolist() == [0, 0, 2, 3] and call["genome_of"].tolist() == [0, 1, 0, 1]
    assert len(pls) == 3 and all("src" not in pl for pl in pls) and [pl["sequences"] for pl in pls] == [4, 4, 4]
    assert nat._lib.freed == 3
    # the static packing alone, and what the binding refuses before the library is asked
    s, d, begin = PangeneNative.pack_edge_lists([])
    assert len(s) == 0 and len(d) == 0 and begin.tolist() == [0]
    with pytest.raises(_lib.PdlError):
        PangeneNative.pack_edge_lists([([1, 2], [3])])
    with pytest.raises(_lib.PdlError):
        nat.placement_batch_of_edges(base, genome_of, [2, 1], lists)                          # one count per list
    with pytest.raises(_lib.PdlError):
        nat.placement_batch_of_edges(base, genome_of[:3], [2, 1, 3], lists)                   # a base of other genes
    assert len(nat._lib.calls) == 1
    nat._ctx = None


def test_the_command_refuses_labels_before_the_device_is_touched(tmp_path, capsys, monkeypatch):
    from pandelos_amd import pangene_native
    from pandelos_amd import place_batch as PB

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(pangene_native.PangeneNative, "open", classmethod(no_device))
    base = _write(tmp_path / "base.faa", [(b"A", b"a1", b"ACDEFG"), (b"B", b"b1", b"CDEFGH")])
    clash = _write(tmp_path / "clash.faa", [(b"X", b"x1", b"ACDEFG"), (b"B", b"q1", b"ACDEFG")])
    one = _write(tmp_path / "one.faa", [(b"X", b"x1", b"ACDEFG")])
    unsafe = _write(tmp_path / "unsafe.faa", [(b"../X", b"x1", b"ACDEFG")])
    out = tmp_path / "out"
    run = lambda *q: PB.main(["-i", str(base), "-k", "3", *[a for f in q for a in ("-q", str(f))], "--out-dir", str(out), "--net"])
    assert run(clash) == 2 and "already names a base genome" in capsys.readouterr().err
    assert run(one, one) == 2 and "each query is one genome of one file" in capsys.readouterr().err
    assert run(one, unsafe) == 2 and "not a safe file name" in capsys.readouterr().err
    assert not out.exists()
    with pytest.raises(AssertionError, match="the device was touched"):
        run(one)
