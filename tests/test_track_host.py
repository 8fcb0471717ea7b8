"""Host-side checks of the track calls (mk_track_text / mk_track_device): header, binding, report formats and CLI layers.
No kernel is launched here; tests/test_gpu_track.py tracks on the GPU."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from mercat2_amd import cli, kmers, native, report

HEADER = (ROOT / "include" / "mercat_hip.h").read_text()
CTYPE = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int32_t": C.c_int32, "double": C.c_double}


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


def _layout(name):
    """(size, alignment, [(field, offset)]) of a header struct by the C rules: every field at the next multiple of its
    alignment, the size a multiple of the largest."""
    at, align, fields = 0, 1, []
    for ctype, field in _struct_fields(name):
        size, al = (_layout(ctype)[:2] if ctype.startswith("mk_") else (C.sizeof(CTYPE[ctype]),) * 2)
        at = (at + al - 1) // al * al
        fields.append((field, at))
        at += size
        align = max(align, al)
    return (at + align - 1) // align * align, align, fields


def test_header_declares_the_calls_and_flags():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ("mk_track_text", "mk_track_device"):
        assert re.search(r"\bint %s\s*\(mk_ctx\*" % name, code)
        assert name in native.ABI_SYMBOLS and getattr(native.lib(), name) is not None
    assert re.search(r"#define MK_TRACK_FOLD\s+1u", code) and re.search(r"#define MK_TRACK_SAT32\s+2u", code)
    assert native.TRACK_FOLD == native.SCREEN_FOLD == 1 and native.TRACK_SAT32 == 2
    # both prototypes take what the issue's ABI lists, in its order
    args = re.search(r"int mk_track_text\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "ctx", "text", "n", "piece_bytes", "flags", "at_least", "counts", "counts_cap", "nwindows", "offsets", "median", "rows", "cap",
        "nrows", "st"]
    args = re.search(r"int mk_track_device\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "ctx", "d_text", "n", "flags", "at_least", "d_counts", "counts_cap", "nwindows", "d_offsets", "d_median", "d_rows", "cap", "nrows",
        "st"]
    assert len(native.lib().mk_track_text.argtypes) == 15 and len(native.lib().mk_track_device.argtypes) == 14
    # the track block follows the filter block
    assert code.index("mk_filter_device") < code.index("MK_TRACK_FOLD") < code.index("mk_track_text") < code.index("mk_merged_export")


def test_bound_struct_matches_the_header():
    want_size, _, want = _layout("mk_track_t")
    assert [f for f, _ in want] == [g[0] for g in native.Track._fields_]
    assert [(f, getattr(native.Track, f).offset) for f, _ in want] == want
    assert C.sizeof(native.Track) == want_size == 96 + 16 + 32 == 144
    for (ctype, field), (_, got) in zip(_struct_fields("mk_track_t"), native.Track._fields_):
        assert got is (native.Screen if ctype == "mk_screen_t" else CTYPE[ctype]), field
    assert _struct_fields("mk_track_t")[0] == ("mk_screen_t", "screen") and native.Track.screen.offset == 0
    st = native.Track()
    st.screen.records, st.windows_out, st.saturated, st.s_track = 7, 99, 3, 0.5
    d = st.as_dict()
    assert d["records"] == 7 and d["windows_out"] == 99 and d["saturated"] == 3 and d["s_track"] == 0.5
    assert {"s_place", "s_median", "s_write", "s_parse", "s_probe", "headless", "pieces"} <= set(d)


def test_the_abi_number_stands():
    assert native.MK_ABI == 6 and native.lib().mk_version().decode().split()[1].split(".")[0] == "6"


def test_python_layers_are_there():
    for name in ("track", "track_device"):
        assert callable(getattr(native.Counter, name))
    assert callable(kmers.track_reads) and "FASTQ" in kmers.track_reads.__doc__ and "fq2fa" in kmers.track_reads.__doc__
    for name in ("format_track_txt", "write_track_txt", "write_track_median_tsv"):
        assert callable(getattr(report, name))


def test_track_txt_format(tmp_path):
    names = ["r1", "", "none", "last"]
    counts = np.array([3, 0, 18446744073709551615, 7, 1, 1], dtype=np.uint64)
    offsets = np.array([0, 3, 4, 4, 6], dtype=np.uint64)
    want = b">r1\n3 0 18446744073709551615\n>\n7\n>none\n\n>last\n1 1\n"
    assert report.format_track_txt(names, counts, offsets) == want
    assert report.write_track_txt(tmp_path / "t.txt", names, counts, offsets) == 4 and (tmp_path / "t.txt").read_bytes() == want
    assert report.format_track_txt(names, counts.astype(np.uint32)[[0, 1, 3, 3, 4, 5]], offsets).startswith(b">r1\n3 0 7\n")
    assert report.format_track_txt([], counts[:0], offsets[:1]) == b""
    with pytest.raises(ValueError):
        report.format_track_txt(names[:3], counts, offsets)


def test_median_tsv_format(tmp_path):
    names = ["r1", "", "none"]
    rows = np.array([[3, 2, 18446744073709551615, 0, 18446744073709551612], [1, 1, 7, 7, 7], [0, 0, 0, 0, 0]], dtype=np.uint64)
    median = np.array([3, 7, 0], dtype=np.uint64)
    want = (b"record\twindows\tmedian\tsum\tmin\tmax\n"
            b"r1\t3\t3\t18446744073709551615\t0\t18446744073709551612\n\t1\t7\t7\t7\t7\nnone\t0\t0\t0\t0\t0\n")
    assert report.write_track_median_tsv(tmp_path / "m.tsv", names, rows, median) == 3 and (tmp_path / "m.tsv").read_bytes() == want
    with pytest.raises(ValueError):
        report.write_track_median_tsv(tmp_path / "x.tsv", names, rows, median[:2])


def test_cli_accepts(tmp_path):
    fasta = str(GOLDEN / "inputs" / "A.fasta")
    args, _ = cli.parseargs(["-i", fasta, "-k", "5", "-track", fasta])
    assert (args.track, args.track_kind, args.track_sat32) == (fasta, "nucleotide", False)
    assert cli.parseargs(["-i", fasta, "-k", "5", "-track", fasta, "-track_sat32"])[0].track_sat32 is True
    for name, kind in (("x.faa.gz", "protein"), ("x.fastq.gz", "nucleotide"), ("x.fq", "nucleotide"), ("x.fna", "nucleotide")):
        (tmp_path / name).write_bytes(b"")
        assert cli.parseargs(["-i", fasta, "-k", "5", "-track", str(tmp_path / name)])[0].track_kind == kind
    args, _ = cli.parseargs(["-i", fasta, "-k", "5"])
    assert args.track is None and args.track_kind is None and args.track_sat32 is False


def test_cli_rejects(tmp_path, capsys):
    fasta = str(GOLDEN / "inputs" / "A.fasta")
    out = tmp_path / "out"
    for extra in (["-track", str(tmp_path / "missing.fa")], ["-track", str(ROOT / "README.md")], ["-track_sat32"]):
        with pytest.raises(SystemExit) as e:
            cli.main(["-i", fasta, "-k", "5", "-o", str(out)] + extra)
        assert e.value.code == 2 and not out.exists(), extra  # (before the output folder is made, before any counting)
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        cli.parseargs(["-h"])
    text = " ".join(capsys.readouterr().out.split())
    assert e.value.code == 0 and "-track FILE" in text and "-track_sat32" in text and "_median.tsv" in text
