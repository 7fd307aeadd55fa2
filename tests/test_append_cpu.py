"""pdl_append_genomes without a GPU: the binding agrees with the header, both libraries export the symbol, the append command
refuses what the union cannot mean before any device call, and the seed range of the GPU fuzz test is not mostly skipped."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

from pandelos_amd.pangene_idata import PangeneIData

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "pandelos_amd" / "lib"
APPEND_SEED0, APPEND_SEEDS_DEFAULT = 7000, 120        # the range tests/test_gpu_append.py runs by default


def test_append_info_matches_the_header(tmp_path):
    from pandelos_amd import _lib
    src, exe = tmp_path / "size.c", tmp_path / "size"
    src.write_text('#include <stdio.h>\n#include "pandelos_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(pdl_append_info), offsetof(pdl_append_info, rank_sort_ms), '
                   'offsetof(pdl_append_info, device_ms)); return 0; }\n')
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    size, off_rank, off_dev = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert C.sizeof(_lib.PdlAppendInfo) == size
    assert _lib.PdlAppendInfo.rank_sort_ms.offset == off_rank and _lib.PdlAppendInfo.device_ms.offset == off_dev
    assert "pdl_append_genomes" in _lib.EXPORTS


@pytest.mark.parametrize("lib", ["libpandelos_amd.so", "libnative.so"])
def test_libraries_export_the_symbol(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB / lib)], check=True, capture_output=True, text=True).stdout
    assert any(line.split()[-1] == "pdl_append_genomes" for line in out.splitlines() if line.strip())


def _write(path, recs):
    path.write_bytes(b"".join(b"%s\t%s\tp\n%s\n" % r for r in recs))


def test_append_command_refuses_a_label_clash_and_an_empty_file(tmp_path, capsys, monkeypatch):
    from pandelos_amd import append as A
    from pandelos_amd import pangene_native
    base, new, clash, again, empty = (tmp_path / n for n in ("base.faa", "new.faa", "clash.faa", "again.faa", "empty.faa"))
    _write(base, [(b"A", b"a1", b"ACDEFG"), (b"B", b"b1", b"CDEFGH")])
    _write(new, [(b"X", b"x1", b"ACDEFG"), (b"Y", b"y1", b"CDEFGH")])
    _write(clash, [(b"Z", b"z1", b"ACDEFG"), (b"B", b"q1", b"ACDEFG")])
    _write(again, [(b"X", b"x2", b"ACDEFG")])
    empty.write_bytes(b"\n")

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the labels were checked")
    monkeypatch.setattr(pangene_native.PangeneNative, "open", staticmethod(no_device))
    out = tmp_path / "union.net"
    assert A.main(["-i", str(base), "-k", "3", "-a", str(clash), "-o", str(out)]) == 2
    assert "'B' already names a genome" in capsys.readouterr().err
    # a label of an EARLIER appended file clashes too: by then it names a genome of the context
    assert A.main(["-i", str(base), "-k", "3", "-a", str(new), "-a", str(again), "-o", str(out)]) == 2
    assert "'X' already names a genome" in capsys.readouterr().err
    assert A.main(["-i", str(base), "-k", "3", "-a", str(empty), "-o", str(out)]) == 2
    assert "no gene" in capsys.readouterr().err
    assert not out.exists()
    with pytest.raises(A.AppendError):
        A.check_append(PangeneIData.read_from_file(clash), ["A", "B"])
    A.check_append(PangeneIData.read_from_file(new), ["A", "B"])          # several new genomes in one file are fine
    with pytest.raises(SystemExit):                                        # argparse: -a is required
        A.main(["-i", str(base), "-k", "3", "-o", str(out)])


def test_the_fuzz_seed_range_is_mostly_usable():
    """tests/test_gpu_append.py skips the seeds whose set has no usable split (one genome only, a base without a k-mer, a
    newcomer letter the base lacks); at most a quarter of the default range may be skipped."""
    from tests.test_gpu_query import _random_case
    skipped = sum(_random_case(seed) is None for seed in range(APPEND_SEED0, APPEND_SEED0 + APPEND_SEEDS_DEFAULT))
    assert 4 * skipped <= APPEND_SEEDS_DEFAULT, f"{skipped} of {APPEND_SEEDS_DEFAULT} seeds give no usable split"
