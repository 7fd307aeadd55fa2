"""bench.py is what the driver runs: ONE JSON line with the contract's fields, on one GPU and — started by the script itself when
no launcher did — on N ranks (here: two ranks rehearsed on the one device over gloo, which walks the same N > 1 flow: senders'
range tuples, the three exchanges, per-rank results reduced).  A plain run times its steps and nothing else; --full adds the
figures that take runs of their own; --dump-outputs writes the Scores blocks of the last timed step."""
import hashlib
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from pandelos_amd.scores import FIELDS
from tests import helpers as H

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
ROOT = Path(__file__).resolve().parents[1]

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
            "data", "config", "roofline")


def _bench(*args):
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], cwd=ROOT, capture_output=True, text=True, timeout=800)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip() and not l.startswith("[Gloo]")]      # (the rehearsal's transport announces itself on stdout)
    assert len(lines) == 1, f"bench.py must print ONE line, got {len(lines)}"
    return json.loads(lines[0])


def test_default_run_prints_the_contract_line():
    d = _bench("--full")
    for k in CONTRACT + ("cpu_baseline", "value_host_to_host", "pipeline", "stage_ms", "roofline_whole_path"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["higher_is_better"] is True and d["vs_baseline"] is None and d["data"].startswith("synthetic")
    assert d["metric"] and d["unit"] == "gene-pairs/s" and "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] * d["ms_per_step"] / 1e3 / (d["config"]["genes"] * (d["config"]["genes"] - 1)) - 1) < 1e-6      # value = pairs / step time
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert 0.05 < r["frac"] < 1.0 and (r["traffic"] is None or r["traffic"] > r["bytes_per_launch"] * 0.5)
    c = d["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0 and c["sample"]
    assert d["stage_ms"]["aside_reloads"] == 0 and d["value_host_to_host"] < d["value"]
    assert d["pipeline"]["faa_to_net_ms"] > d["pipeline"]["dictionary_ms"] > 0


def test_two_ranks_print_the_contract_line():
    d = _bench("--gpus", "2", "--steps", "3", "--warmup", "1", "--full")
    for k in CONTRACT:
        assert k in d, k
    import torch
    assert d["n_gpus"] == 2 and d["scaling"] == "strong"
    assert bool(d.get("rehearsal", False)) == (torch.cuda.device_count() < 2)        # (a box with two GPUs runs the two ranks over RCCL for real)
    st = d["stage_ms"]
    assert st["range_lists_by"] == "senders" and st["dist_ranges"] > 0 and st["dist_finish"] > 0 and st["aside_reloads"] == 0
    assert d["scale_set"]["n_gpus"] == 2 and d["scale_set"]["emitted_cells"] == 55236320       # (configs[3]: the reference's count, summed over the ranks)


def _genome_blocks(out_dir, genes_of_genome):
    """bench.py --dump-outputs files -> per-genome Scores fields with the library's dtypes again."""
    arr = {f: np.load(out_dir / f"{f}.npy") for f in FIELDS + ("scoresCount",)}
    counts = arr["scoresCount"].astype(np.int64)
    G, N = len(genes_of_genome), int(genes_of_genome.sum())
    cut = lambda a, sizes: np.split(a, np.cumsum(sizes)[:-1])
    per = {f: cut(arr[f], counts) for f in ("scores", "percs", "tr_percs", "row", "column", "first_seq_genome", "second_seq_genome")}
    per["max_genome_score"] = cut(arr["max_genome_score"].reshape(N, G), genes_of_genome)
    per["max_genome_score_col"] = cut(arr["max_genome_score_col"], [N] * G)
    per["scoresMaxMappings"] = cut(arr["scoresMaxMappings"], [N] * G)
    ints = ("row", "column", "first_seq_genome", "second_seq_genome", "scoresMaxMappings")
    return counts, [{f: per[f][g].astype(np.int32 if f in ints else np.float32) for f in FIELDS} for g in range(G)]


def test_plain_run_times_its_steps_and_dumps_the_reference_outputs(tmp_path):
    """The plain run: the headline fields, none of --full's; its dump = the reference's Scores of the 64-genome set
    (tests/golden/digests_baseline.json), field for field."""
    d = _bench("--steps", "4", "--warmup", "1", "--dump-outputs", str(tmp_path))
    for k in CONTRACT + ("roofline_whole_path",):
        assert k in d, k
    for k in ("cpu_baseline", "host_path", "host_path_native", "pipeline", "scale_set", "stage_ms"):
        assert k not in d, k
    assert d["steps"] == 4 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["roofline"]["traffic"] is None
    assert abs(d["value"] * d["ms_per_step"] / 1e3 / (d["config"]["genes"] * (d["config"]["genes"] - 1)) - 1) < 1e-6
    ref = json.loads((H.GOLDEN / "digests_baseline.json").read_text())["mycoplasma64_standin"]
    assert d["config"]["k"] == ref["k"] and d["config"]["genes"] == ref["sequences"]
    assert sum(p.stat().st_size for p in tmp_path.iterdir()) <= 64_000_000
    gs = H.make_gene_set(**ref["shape"])
    counts, blocks = _genome_blocks(tmp_path, np.bincount(gs.genome_of.astype(np.int64), minlength=ref["genomes"]))
    assert list(counts) == ref["scoresCount"]
    for g, b in enumerate(blocks):
        for f in FIELDS:
            assert hashlib.sha256(H.raw(b[f]).tobytes()).hexdigest() == ref["sha256"][g][f], f"genome {g} field {f}"
