"""Host side of the abundance histogram (mk_histo / mk_histo_device, Counter.histo*, report.format_histo, the -histo flag): the
binding, the ABI number, the argument parser and the formatters.  No GPU is touched."""
import ctypes
import re
import subprocess
from pathlib import Path

import pytest

from mercat2_amd import cli, native, report

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).parent / "golden"
SYMBOLS = ("mk_histo", "mk_histo_device")


def test_header_binding_and_library_agree_on_the_histogram():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mercat_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(mk_[a-z0-9_]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared and name in native.ABI_SYMBOLS and getattr(native.lib(), name) is not None


def test_histo_struct_layout(tmp_path):
    assert ctypes.sizeof(native.Histo) == 64 == 6 * 8 + 2 * 8
    assert [n for n, _ in native.Histo._fields_] == ["distinct", "total", "max_count", "over_rows", "over_total", "slots",
                                                      "s_scan", "s_total"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mercat_hip.h"\n'
                   'int main(){printf("%zu %zu %zu",sizeof(mk_histo_t),offsetof(mk_histo_t,over_total),offsetof(mk_histo_t,s_scan));return 0;}\n')
    subprocess.check_call(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(tmp_path / "sz")])
    assert subprocess.check_output([str(tmp_path / "sz")]).decode().split() == [
        "64", str(native.Histo.over_total.offset), str(native.Histo.s_scan.offset)]


def test_abi_number_stays():
    assert native.MK_ABI == 6
    assert native.lib().mk_version().decode() == "mercat_hip 6.1 (gfx950)"


def test_format_histo_on_hand_written_bins():
    bins = [0, 7, 0, 0, 2, 0, 18446744073709551615]  # high = 5: bin 6 is the overflow bin
    assert report.format_histo(bins) == b"1 7\n4 2\n6 18446744073709551615\n"
    assert report.format_histo(bins, full=True) == b"1 7\n2 0\n3 0\n4 2\n5 0\n6 18446744073709551615\n"
    assert report.format_histo(bins, True).endswith(b"\n6 18446744073709551615\n")
    assert report.format_histo([0, 0, 0, 0]) == b""
    assert report.format_histo([0, 0, 3]) == b"2 3\n"  # high = 1: only the overflow line
    import numpy as np
    assert report.format_histo(np.array(bins, dtype=np.uint64)) == report.format_histo(bins)


def test_format_histo_tsv_rows_where_any_sample_has_one():
    a, b = [0, 5, 0, 0, 1, 0], [0, 0, 0, 2, 1, 9]
    assert report.format_histo_tsv(["b", "a"], [b, a]) == b"count\tb\ta\n1\t0\t5\n3\t2\t0\n4\t1\t1\n5\t9\t0\n"
    assert report.format_histo_tsv(["only"], [[0, 0, 0]]) == b"count\tonly\n"


def _result_folder(tmp_path, k=5):
    out = tmp_path / "old"
    (out / "tsv_nucleotide").mkdir(parents=True)
    (out / "tsv_nucleotide" / "s1_counts.tsv").write_bytes(b"k-mer\ts1_Count\n" + b"A" * k + b"\t12\n")
    return out


def test_parseargs_accepts_histo(tmp_path, capsys):
    fasta = str(GOLDEN / "inputs" / "A.fasta")
    args, _ = cli.parseargs(["-i", fasta, "-k", "5"])
    assert args.histo is None
    args, _ = cli.parseargs(["-i", fasta, "-k", "5", "-histo"])
    assert args.histo == 10000
    args, _ = cli.parseargs(["-k", "5", "-histo", "255", "-i", fasta])
    assert args.histo == 255
    args, _ = cli.parseargs(["-k", "5", "-histo", "1048576", "-i", fasta])
    assert args.histo == 1 << 20
    args, _ = cli.parseargs(["-tsv", str(_result_folder(tmp_path)), "-k", "5", "-histo"])
    assert args.histo == 10000 and args.i == [] and sorted(args.loaded["nucleotide"]) == ["s1"]
    for bad in ("0", "1048577", "-3"):
        with pytest.raises(SystemExit) as e:
            cli.parseargs(["-i", fasta, "-k", "5", "-histo", bad])
        assert e.value.code == 2
        capsys.readouterr()


def test_python_layers_are_there():
    for name in ("histo", "histo_device"):
        assert callable(getattr(native.Counter, name))
    assert callable(native.histo_multi) and "overlap" in native.histo_multi.__doc__
    assert callable(report.write_histo_files) and callable(report.write_histo_tsv)


def test_no_new_environment_switch():
    text = (ROOT / "mercat2_amd" / "csrc" / "mk_histo.hip").read_text()
    assert not re.search(r"\b(getenv|mk_env_\w+)\s*\(", text)
    assert re.search(r"^#define\s+HS_WINDOW\s+\d+\s*$", text, flags=re.M)
