"""bench.py --dump-outputs: the files write_outputs() makes from Scores blocks (no GPU: blocks of the C oracle)."""
import numpy as np

import bench
from oracle import binding as ob
from pandelos_amd.scores import FIELDS
from pandelos_amd.synth import make_gene_set

SHAPE = dict(genomes=5, genes_per_genome=60, mean_len=80, sub_rate=0.08, seed=1)


def _blocks():
    gs = make_gene_set(**SHAPE)
    o = ob.Oracle(gs.residues, gs.offsets, gs.genome_of, 3)
    return {g: o.scores(g) for g in range(o.genomes)}


def test_every_field_is_written_whole_in_genome_order(tmp_path):
    blocks = _blocks()
    bench.write_outputs(blocks, tmp_path)
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted([f"{f}.npy" for f in FIELDS] + ["scoresCount.npy"])
    counts = np.load(tmp_path / "scoresCount.npy")
    assert counts.dtype == np.float64 and list(counts) == [blocks[g]["scoresCount"] for g in range(len(blocks))]
    for f in FIELDS:
        got = np.load(tmp_path / f"{f}.npy")
        want = np.concatenate([np.asarray(blocks[g][f]) for g in range(len(blocks))])
        assert got.dtype in (np.float32, np.float64) and got.shape == want.shape, f
        assert np.array_equal(got.astype(want.dtype), want), f                  # integers come back exactly
    assert np.load(tmp_path / "scoresMaxMappings.npy").dtype == np.float64    # (holds 2^31 - 1: not exact in float32)


def test_a_large_output_is_cut_to_the_same_seeded_sample(tmp_path, monkeypatch):
    blocks = _blocks()
    whole = tmp_path / "whole"
    bench.write_outputs(blocks, whole)
    monkeypatch.setattr(bench, "DUMP_LIMIT", 40_000)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.write_outputs(blocks, a)
    bench.write_outputs(blocks, b)
    assert sum(p.stat().st_size for p in a.iterdir()) <= 40_000
    for p in a.iterdir():
        assert p.read_bytes() == (b / p.name).read_bytes(), p.name
    for f in FIELDS:
        idx = np.load(a / f"{f}.index.npy").astype(np.int64)
        assert len(idx) > 0 and np.all(np.diff(idx) > 0)
        assert np.array_equal(np.load(a / f"{f}.npy"), np.load(whole / f"{f}.npy").reshape(-1)[idx]), f
    assert np.array_equal(np.load(a / "scoresCount.npy"), np.load(whole / "scoresCount.npy"))
