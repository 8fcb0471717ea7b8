"""Host-side checks of the screen calls (mk_screen_text / mk_screen_device): header, binding, report and CLI layers.
No kernel is launched here; tests/test_gpu_screen.py screens on the GPU."""
import ctypes as C
import io
import re
from pathlib import Path

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, read_input
from mercat2_amd import cli, kmers, native, report

HEADER = (ROOT / "include" / "mercat_hip.h").read_text()


def _struct_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if stmt:
            ctype, rest = stmt.split(" ", 1)
            out += [(ctype, f.strip()) for f in rest.split(",")]
    return out


def test_header_declares_the_calls_and_structs():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ("mk_screen_text", "mk_screen_device"):
        assert re.search(r"\bint %s\s*\(mk_ctx\*" % name, code)
        assert name in native.ABI_SYMBOLS and getattr(native.lib(), name) is not None
    assert re.search(r"#define MK_SCREEN_FOLD 1u", code) and native.SCREEN_FOLD == native.LOOKUP_FOLD == 1
    assert [f for _, f in _struct_fields("mk_screen_row_t")] == list(native.SCREEN_COLUMNS) == ["windows", "hits", "sum", "min", "max"]


@pytest.mark.parametrize("cname,cls", [("mk_screen_row_t", "ScreenRow"), ("mk_screen_t", "Screen")])
def test_bound_structs_match_the_header(cname, cls, tmp_path):
    ctype = {"uint64_t": C.c_uint64, "int32_t": C.c_int32, "double": C.c_double}
    want = _struct_fields(cname)
    got = getattr(native, cls)._fields_
    assert [f for _, f in want] == [g[0] for g in got]
    assert all(gt is ctype[t] for (t, _), (_, gt) in zip(want, got))
    assert C.sizeof(getattr(native, cls)) == sum(C.sizeof(ctype[t]) for t, _ in want)  # (no padding: 8-byte fields, int32 in pairs)
    assert C.sizeof(native.ScreenRow) == 40 == 8 * len(native.SCREEN_COLUMNS)


def test_the_abi_number_stands():
    assert native.MK_ABI == 6 and native.lib().mk_version().decode().split()[1].split(".")[0] == "6"


def test_python_layers_are_there():
    for name in ("screen", "screen_device"):
        assert callable(getattr(native.Counter, name))
    assert callable(kmers.screen_reads) and callable(kmers.record_names) and callable(report.write_screen_tsv)
    # a table spread by key range cannot give `min` from per-range rows (a window absent from one range is not absent
    # from the table): no screen_multi rather than a wrong one
    assert not hasattr(native, "screen_multi")


def test_write_screen_tsv_formatting(tmp_path):
    rows = np.array([[6, 4, 10, 1, 2], [0, 0, 0, 0, 0], [1, 1, 2**64 - 1, 2**64 - 1, 2**64 - 1]], dtype=np.uint64)
    assert report.write_screen_tsv(tmp_path / "s.tsv", ["a", "", "r|3"], rows) == 3
    assert (tmp_path / "s.tsv").read_bytes() == (b"record\twindows\thits\tsum\tmin\tmax\na\t6\t4\t10\t1\t2\n\t0\t0\t0\t0\t0\n"
                                                 b"r|3\t1\t1\t18446744073709551615\t18446744073709551615\t18446744073709551615\n")
    assert report.format_screen_tsv([], np.zeros((0, 5), dtype=np.uint64)) == b"record\twindows\thits\tsum\tmin\tmax\n"
    with pytest.raises(ValueError):
        report.format_screen_tsv(["a"], rows)


def _reference_names(text: bytes):
    """The reference's line loop (lib/mercat2_kmers.py:49-69) naming its records: text mode, strip(), startswith('>')."""
    names, headless = [], False
    for line in io.TextIOWrapper(io.BytesIO(text), encoding="utf-8", errors="replace", newline=None):
        line = line.strip()
        if line.startswith(">"):
            words = line[1:].split()
            names.append(words[0] if words else "")
        elif not names and line.replace("*", ""):
            headless = True
    return ([""] if headless else []) + names


EDGE = sorted(p.name for p in (GOLDEN / "inputs").glob("edge_*")) + ["A.fasta", "Test_R1.fna.gz"]


@pytest.mark.parametrize("name", EDGE)
def test_record_names_follow_the_reference_line_loop(name):
    text = read_input(name)
    assert kmers.record_names(text) == _reference_names(text)


def test_record_names_of_odd_texts():
    cases = [b"", b"\n\n", b"ACGT", b"  \n***\n>a\n", b" \x0b\nAC\n>a b\n>  \n>\tc d\r>e\r\nAC>GT\n", b">a\x0bb\nAC\x0cGT\n\x1c>f\n",
             b"*\nA*\n>x", b">a \xc3\xa9\n"]
    for text in cases:
        assert kmers.record_names(text) == _reference_names(text), text
    assert kmers.record_names(b" \x0b\nAC\n>a b\n>  \n>\tc d\r>e\r\nAC>GT\n") == ["", "a", "", "c", "e"]


def test_cli_argument_errors(tmp_path, capsys):
    fasta = str(GOLDEN / "inputs" / "A.fasta")
    out = tmp_path / "out"
    bad = [["-screen", str(tmp_path / "missing.fa")], ["-screen", fasta, "-screen_min", "0"], ["-screen", fasta, "-screen_min", "-3"],
           ["-screen", fasta, "-screen_min", "x"], ["-screen", str(ROOT / "README.md")]]
    for extra in bad:
        with pytest.raises(SystemExit) as e:
            cli.main(["-i", fasta, "-k", "5", "-o", str(out)] + extra)
        assert e.value.code == 2 and not out.exists()  # (before the output folder is made, before any counting)
    capsys.readouterr()
    args, _ = cli.parseargs(["-i", fasta, "-k", "5", "-screen", fasta])
    assert args.screen_kind == "nucleotide" and args.screen_min == 1
    for name, kind in (("x.faa.gz", "protein"), ("x.fastq.gz", "nucleotide"), ("x.fq", "nucleotide"), ("x.fna", "nucleotide")):
        (tmp_path / name).write_bytes(b"")
        assert cli.parseargs(["-i", fasta, "-k", "5", "-screen", str(tmp_path / name), "-screen_min", "7"])[0].screen_kind == kind
