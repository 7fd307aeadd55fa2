"""pdl_query_batch without a GPU: the command's splitting of query files into genomes and its label refusals, the gene_begin
packing of PangeneNative.query_batch against a stub library, and the header's declaration."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from pandelos_amd.pangene_idata import PangeneIData

ROOT = Path(__file__).resolve().parents[1]


def _write(path, recs):
    path.write_bytes(b"".join(b"%s\t%s\tp %s\n%s\n" % (g, n, n, s) for g, n, s in recs))
    return path


def test_a_query_file_is_split_into_its_genomes_in_first_seen_order(tmp_path):
    from pandelos_amd.query_batch import split_genomes
    f = _write(tmp_path / "q.faa", [(b"X", b"x1", b"ACDEFG"), (b"Y", b"y1", b"CDEFGH"), (b"X", b"x2", b"DEFGHI"), (b"Z", b"z1", b"EF"),
                                    (b"Y", b"y2", b"FGHIKL")])
    parts = split_genomes(PangeneIData.read_from_file(f))
    assert [p.genomeNames for p in parts] == [["X"], ["Y"], ["Z"]]
    assert [p.sequenceName for p in parts] == [["x1", "x2"], ["y1", "y2"], ["z1"]]
    assert [p.sequences for p in parts] == [[b"ACDEFG", b"DEFGHI"], [b"CDEFGH", b"FGHIKL"], [b"EF"]]
    assert parts[1].sequenceDescription == ["p y1", "p y2"]
    assert all(set(p.sequenceGenome) == {0} for p in parts)
    # a part is what reading that genome's records alone gives
    alone = PangeneIData.read_from_file(_write(tmp_path / "y.faa", [(b"Y", b"y1", b"CDEFGH"), (b"Y", b"y2", b"FGHIKL")]))
    assert parts[1] == alone


def test_queries_are_collected_over_several_files_and_labels_are_checked(tmp_path):
    from pandelos_amd.query import QueryError
    from pandelos_amd.query_batch import check_label, collect_queries
    a = PangeneIData.read_from_file(_write(tmp_path / "a.faa", [(b"X", b"x1", b"ACDEFG"), (b"Y", b"y1", b"CDEFGH")]))
    b = PangeneIData.read_from_file(_write(tmp_path / "b.faa", [(b"Z", b"z1", b"ACDEFG")]))
    got = collect_queries([("a.faa", a), ("b.faa", b)], ["A", "B"])
    assert [label for label, _ in got] == ["X", "Y", "Z"]
    assert [d.sequenceName for _, d in got] == [["x1"], ["y1"], ["z1"]]
    with pytest.raises(QueryError, match="already names a base genome"):
        collect_queries([("a.faa", a)], ["A", "Y"])
    with pytest.raises(QueryError, match="is in 'a.faa' and in 'c.faa'"):
        collect_queries([("a.faa", a), ("c.faa", a)], ["A"])
    with pytest.raises(QueryError, match="holds no genome"):
        collect_queries([("e.faa", PangeneIData())], ["A"])
    for bad in ("", ".", "..", ".hidden", "-rf", "a/b", "..\\x", "a b", "x\n", "nul\0", "é", "x" * 201, "a:b", "~root", "$HOME", "*"):
        with pytest.raises(QueryError, match="not a safe file name"):
            check_label(bad)
    for good in ("X", "GCF_000027325.1", "strain-7+a=b,c@d", "0", "_x"):
        check_label(good)


def test_the_command_refuses_labels_before_the_device_is_touched(tmp_path, capsys, monkeypatch):
    from pandelos_amd import pangene_native
    from pandelos_amd import query_batch as QB

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(pangene_native.PangeneNative, "open", classmethod(no_device))
    base = _write(tmp_path / "base.faa", [(b"A", b"a1", b"ACDEFG"), (b"B", b"b1", b"CDEFGH")])
    clash = _write(tmp_path / "clash.faa", [(b"X", b"x1", b"ACDEFG"), (b"B", b"q1", b"ACDEFG")])
    one = _write(tmp_path / "one.faa", [(b"X", b"x1", b"ACDEFG")])
    unsafe = _write(tmp_path / "unsafe.faa", [(b"../X", b"x1", b"ACDEFG")])
    out = tmp_path / "out"
    run = lambda *q: QB.main(["-i", str(base), "-k", "3", *[a for f in q for a in ("-q", str(f))], "--out-dir", str(out)])
    assert run(clash) == 2 and "already names a base genome" in capsys.readouterr().err
    assert run(one, one) == 2 and "each query is one genome of one file" in capsys.readouterr().err
    assert run(one, unsafe) == 2 and "not a safe file name" in capsys.readouterr().err
    assert not out.exists()
    with pytest.raises(AssertionError, match="the device was touched"):
        run(one)
    # the single-query command keeps refusing a file of several genomes
    from pandelos_amd import query as Q
    two = _write(tmp_path / "two.faa", [(b"X", b"x1", b"ACDEFG"), (b"Y", b"y1", b"CDEFGH")])
    assert Q.main(["-i", str(base), "-k", "3", "-q", str(two), "-o", str(tmp_path / "n.net")]) == 2
    assert "exactly one genome" in capsys.readouterr().err


class _StubLib:
    """Stands in for libpandelos_amd.so: records what pdl_query_batch was given, answers with blocks that hold no cell."""

    def __init__(self):
        self.calls, self.freed, self.alive = [], 0, []

    def pdl_query_batch(self, ctx, residues, offsets, gene_begin, n, n_queries, out, info, binfo):
        as_np = lambda addr, ct, count: np.ctypeslib.as_array(C.cast(addr, C.POINTER(ct)), shape=(count,)).copy() if count else np.zeros(0)
        off = as_np(offsets, C.c_uint64, n + 1)
        self.calls.append({"residues": as_np(residues, C.c_uint8, int(off[-1])) if residues else np.zeros(0, np.uint8), "offsets": off,
                           "gene_begin": as_np(gene_begin, C.c_uint32, n_queries + 1), "n": n, "n_queries": n_queries})
        for j in range(n_queries):
            out[j].rows, out[j].genomes, out[j].sequences = j + 1, 3, 10 + j
            keep = [np.zeros((j + 1) * 3, np.float32), np.zeros(10 + j, np.float32), np.zeros(10 + j, np.int32)]
            self.alive.append(keep)
            out[j].max_genome_score = keep[0].ctypes.data_as(C.POINTER(C.c_float))
            out[j].max_genome_score_col = keep[1].ctypes.data_as(C.POINTER(C.c_float))
            out[j].scoresMaxMappings = keep[2].ctypes.data_as(C.POINTER(C.c_int32))
            info[j].genome_cost = 100 + j
        b = binfo._obj                                                # (what C.byref wraps)
        b.queries, b.chunks, b.device_ms = n_queries, 2, 1.5
        return 0

    def pdl_free_scores(self, s):
        self.freed += 1

    def pdl_last_error(self, ctx):
        return b"stub"


def test_query_batch_packs_gene_begin_for_the_library():
    from pandelos_amd import _lib
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.__new__(PangeneNative)
    nat._lib, nat._ctx = _StubLib(), None
    q0 = (np.frombuffer(b"ACDEFGHIK", np.uint8), np.array([0, 4, 9], np.uint64))
    q1 = (np.frombuffer(b"xxLMNPQyy", np.uint8), np.array([2, 7], np.uint64))                # offsets that do not start at 0
    q2 = (np.frombuffer(b"RSTVW", np.uint8), [0, 0, 2, 5])                                    # an empty gene, a plain list
    blocks = nat.query_batch([q0, q1, q2])
    call, = nat._lib.calls
    assert call["n"] == 6 and call["n_queries"] == 3
    assert call["gene_begin"].tolist() == [0, 2, 3, 6] and call["gene_begin"].dtype == np.uint32
    assert call["offsets"].tolist() == [0, 4, 9, 14, 14, 16, 19]
    assert call["residues"].tobytes() == b"ACDEFGHIKLMNPQRSTVW"
    assert [b.max_genome_score.shape for b in blocks] == [(1, 3), (2, 3), (3, 3)]
    assert [len(b.max_genome_score_col) for b in blocks] == [10, 11, 12]
    assert nat._lib.freed == 3                                                                # every block goes back to the library
    info = nat.last_query_batch_info
    assert info["chunks"] == 2 and info["device_ms"] == 1.5
    assert [q["genome_cost"] for q in info["queries"]] == [100, 101, 102]
    # the static packing alone, and what it refuses
    res, off, begin = PangeneNative.pack_queries([q1])
    assert res.tobytes() == b"LMNPQ" and off.tolist() == [0, 5] and begin.tolist() == [0, 1]
    with pytest.raises(_lib.PdlError):
        PangeneNative.pack_queries([(q0[0], np.array([0, 5, 3], np.uint64))])
    with pytest.raises(_lib.PdlError):
        PangeneNative.pack_queries([(q0[0], np.array([0, 50], np.uint64))])
    with pytest.raises(ValueError, match="query 1 holds 2"):
        nat.query_batch_idata([PangeneIData.from_arrays(q0[0], q0[1], [0, 0]), PangeneIData.from_arrays(q0[0], q0[1], [0, 1])])
    nat._ctx = None


def test_the_header_declares_pdl_query_batch():
    header = (ROOT / "include" / "pandelos_amd.h").read_text()
    squeeze = lambda s: re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", s, flags=re.S)).strip()
    m = re.search(r"PDL_API\s+int\s+pdl_query_batch\s*\((.*?)\)\s*;", header, flags=re.S)
    assert m, "pdl_query_batch is not declared"
    assert squeeze(m.group(1)) == ("pdl_ctx *, const uint8_t *residues, const uint64_t *offsets , const uint32_t *gene_begin , "
                                   "uint32_t n, uint32_t n_queries, pdl_scores *out , pdl_query_info *info , pdl_query_batch_info *binfo")
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*pdl_query_batch_info\s*;", header)
    assert m and squeeze(m.group(1)) == "uint32_t queries, chunks; float device_ms;"
    from pandelos_amd import _lib
    assert "pdl_query_batch" in _lib.EXPORTS
    assert [(n, C.sizeof(t)) for n, t in _lib.PdlQueryBatchInfo._fields_] == [("queries", 4), ("chunks", 4), ("device_ms", 4)]


@pytest.mark.parametrize("lib", ["libpandelos_amd.so", "libnative.so"])
def test_libraries_export_the_symbol(lib):
    from pandelos_amd import _lib
    assert hasattr(C.CDLL(str(_lib.LIB_DIR / lib)), "pdl_query_batch")
