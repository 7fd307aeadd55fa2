"""Fixtures of pdl_query_scores (tests/golden/query, made by make_golden_query.py from the reference run on the union):
they reproduce through the CPU oracle on the union and — where the reference build exists — through the reference itself;
and the query command refuses what the union cannot mean.  No GPU needed."""
import tempfile
from pathlib import Path

import numpy as np
import pytest

from pandelos_amd.pangene_idata import PangeneIData
from tests import helpers as H

QDIR = H.GOLDEN / "query"
CASES = sorted(p.stem for p in QDIR.glob("*.npz"))


def load_case(name):
    """-> (fixture dict, base PangeneIData, query PangeneIData, k, G)"""
    fx = dict(np.load(QDIR / f"{name}.npz"))
    with tempfile.TemporaryDirectory() as td:
        b, q = Path(td) / "base.faa", Path(td) / "query.faa"
        b.write_bytes(fx["base_faa"].tobytes())
        q.write_bytes(fx["query_faa"].tobytes())
        base, query = PangeneIData.read_from_file(b), PangeneIData.read_from_file(q)
    return fx, base, query, int(fx["k"]), int(fx["G"])


def union_arrays(base, query):
    res_b, off_b, gen_b = base.flatten()
    res_q, off_q, _ = query.flatten()
    G = int(gen_b.max()) + 1
    res = np.concatenate([res_b, res_q])
    off = np.concatenate([off_b, off_b[-1] + off_q[1:]]).astype(np.uint64)
    gen = np.concatenate([gen_b, np.full(len(off_q) - 1, G, np.uint32)]).astype(np.uint32)
    return res, off, gen, G


def assert_block(got: dict, fx: dict, label):
    for f in H.FIELDS:
        have, want = H.raw(np.asarray(got[f])), fx[f]
        assert have.shape == want.shape, f"{label} {f}: shape {have.shape} != {want.shape}"
        assert np.array_equal(have, want), f"{label} {f} differs"


def test_the_fixture_set_is_complete():
    assert len(CASES) >= 11, CASES


@pytest.mark.parametrize("name", CASES)
def test_fixture_reproduces_through_the_oracle_on_the_union(name):
    from oracle import binding as ob
    fx, base, query, k, G = load_case(name)
    res, off, gen, g_union = union_arrays(base, query)
    assert g_union == G
    ora = ob.Oracle(res, off, gen, k)
    assert ora.genomes == G + 1
    assert_block(ora.scores(G), fx, name)
    assert ora.genome_cost(G) == int(fx["genome_cost"])


@pytest.mark.parametrize("name", CASES)
def test_fixture_reproduces_through_the_reference_build(name, tmp_path):
    from oracle import binding as ob
    if not ob.have_reference():
        pytest.skip("no reference build in oracle/_ref")
    fx, _, _, k, G = load_case(name)
    union = tmp_path / "union.faa"
    union.write_bytes(fx["base_faa"].tobytes() + fx["query_faa"].tobytes())
    info = ob.run_harness(ob.REF_SO, union, k, dump=tmp_path / "out.bin")
    ref = ob.read_dump(tmp_path / "out.bin")
    assert ref["genomes"] == G + 1
    assert_block(ref["per_genome"][G], fx, name)
    assert info["genome_cost"][G] == int(fx["genome_cost"])


def _write(path, recs):
    path.write_bytes(b"".join(b"%s\t%s\tp\n%s\n" % r for r in recs))


def test_query_command_refuses_two_genomes_and_a_label_clash(tmp_path, capsys):
    from pandelos_amd import query as Q
    base, two, clash = tmp_path / "base.faa", tmp_path / "two.faa", tmp_path / "clash.faa"
    _write(base, [(b"A", b"a1", b"ACDEFG"), (b"B", b"b1", b"CDEFGH")])
    _write(two, [(b"X", b"x1", b"ACDEFG"), (b"Y", b"y1", b"CDEFGH")])
    _write(clash, [(b"B", b"q1", b"ACDEFG")])
    out = tmp_path / "new.net"
    assert Q.main(["-i", str(base), "-k", "3", "-q", str(two), "-o", str(out)]) == 2
    assert "exactly one genome" in capsys.readouterr().err
    assert Q.main(["-i", str(base), "-k", "3", "-q", str(clash), "-o", str(out)]) == 2
    assert "already names a base genome" in capsys.readouterr().err
    assert not out.exists()
    with pytest.raises(Q.QueryError):
        Q.check_query(PangeneIData.read_from_file(two), ["A", "B"])
