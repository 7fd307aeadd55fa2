#!/usr/bin/env python3
"""Regenerate tests/golden/quality/*.txt (build container only).

.txt = the stdout of the reference's example/quality.py run as a subprocess on (.faa, .clus): the .faa written by
       pandelos_amd.synth for the five shapes of tests/golden/make_golden_net.py, the .clus the committed tests/golden/net/<set>.clus
Only the script's output is stored.
"""
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from pandelos_amd.synth import make_gene_set                      # noqa: E402
from tests.golden.make_golden_net import CASES                    # noqa: E402

NET = Path(__file__).resolve().parent / "net"
OUT = Path(__file__).resolve().parent / "quality"
QUALITY = Path("/root/reference/example/quality.py")


def main():
    OUT.mkdir(exist_ok=True)
    for name, (shape, _) in CASES.items():
        with tempfile.TemporaryDirectory() as td:
            faa = Path(td) / "in.faa"
            make_gene_set(**shape).write_faa(faa)
            p = subprocess.run([sys.executable, str(QUALITY), str(faa), str(NET / f"{name}.clus")], capture_output=True, text=True, check=True)
        (OUT / f"{name}.txt").write_text(p.stdout)
        print(name, len(p.stdout.splitlines()), "lines")


if __name__ == "__main__":
    main()
