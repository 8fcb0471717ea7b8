"""Host-side checks of the filter calls (mk_filter_text / mk_filter_device): header, binding, rule helper and CLI layers.
No kernel is launched here; tests/test_gpu_filter.py filters on the GPU."""
import ctypes as C
import math
import re

import pytest

from conftest import GOLDEN, ROOT
from mercat2_amd import cli, kmers, native

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
    for name in ("mk_filter_text", "mk_filter_device"):
        assert re.search(r"\bint %s\s*\(mk_ctx\*" % name, code)
        assert name in native.ABI_SYMBOLS and getattr(native.lib(), name) is not None
    assert re.search(r"#define MK_FILTER_FOLD\s+1u", code) and re.search(r"#define MK_FILTER_INVERT\s+2u", code)
    assert native.FILTER_FOLD == native.SCREEN_FOLD == 1 and native.FILTER_INVERT == 2
    # both prototypes take what the issue's ABI lists, in its order
    args = re.search(r"int mk_filter_text\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "ctx", "text", "n", "piece_bytes", "flags", "rule", "out", "out_cap", "out_len", "rows", "keep", "cap", "nrows", "st"]
    args = re.search(r"int mk_filter_device\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "ctx", "d_text", "n", "flags", "rule", "d_out", "out_cap", "out_len", "d_rows", "d_keep", "cap", "nrows", "st"]
    assert len(native.lib().mk_filter_text.argtypes) == 14 and len(native.lib().mk_filter_device.argtypes) == 13


@pytest.mark.parametrize("cname,cls,size", [("mk_filter_rule_t", "FilterRule", 24), ("mk_filter_t", "Filter", 96 + 48)])
def test_bound_structs_match_the_header(cname, cls, size):
    bound = getattr(native, cls)
    want_size, _, want = _layout(cname)
    assert [f for f, _ in want] == [g[0] for g in bound._fields_]
    assert [(f, getattr(bound, f).offset) for f, _ in want] == want
    assert C.sizeof(bound) == want_size == size
    for (ctype, field), (_, got) in zip(_struct_fields(cname), bound._fields_):
        assert got is (native.Screen if ctype == "mk_screen_t" else CTYPE[ctype]), field


def test_the_screen_block_inside_is_the_screen_struct():
    assert _struct_fields("mk_filter_t")[0] == ("mk_screen_t", "screen") and native.Filter.screen.offset == 0
    assert C.sizeof(native.Screen) == _layout("mk_screen_t")[0] == 96
    st = native.Filter()
    st.screen.records, st.records_out, st.bytes_out, st.preamble, st.s_gather = 7, 3, 99, 5, 0.5
    d = st.as_dict()
    assert d["records"] == 7 and d["records_out"] == 3 and d["bytes_out"] == 99 and d["preamble"] == 5 and d["s_gather"] == 0.5
    assert {"s_place", "s_write", "s_parse", "s_probe", "headless", "pieces"} <= set(d)


def test_the_abi_number_stands():
    assert native.MK_ABI == 6 and native.lib().mk_version().decode().split()[1].split(".")[0] == "6"


def test_python_layers_are_there():
    for name in ("filter", "filter_device"):
        assert callable(getattr(native.Counter, name))
    assert callable(kmers.filter_reads) and callable(native.ppm_of_fraction)
    assert "FASTA" in kmers.filter_reads.__doc__ and "fq2fa" in kmers.filter_reads.__doc__


def test_fraction_to_ppm():
    assert native.ppm_of_fraction(0) == 0 and native.ppm_of_fraction(1) == 1_000_000 and native.ppm_of_fraction(1.0) == 1_000_000
    assert native.ppm_of_fraction(0.5) == 500_000 and native.ppm_of_fraction(1e-6) == 1
    assert native.ppm_of_fraction(0.9999996) == 1_000_000 and native.ppm_of_fraction(4e-7) == 0
    for bad in (-1e-9, 1.0000001, 2, -1, math.nan, math.inf):
        with pytest.raises(ValueError):
            native.ppm_of_fraction(bad)


def test_cli_accepts(tmp_path):
    fasta = str(GOLDEN / "inputs" / "A.fasta")
    args, _ = cli.parseargs(["-i", fasta, "-k", "5", "-filter", fasta])
    assert (args.filter_kind, args.filter_min, args.filter_hits, args.filter_frac, args.filter_keep) == ("nucleotide", 1, 1, 0.0, "unmatched")
    args, _ = cli.parseargs(["-i", fasta, "-k", "5", "-filter", fasta, "-filter_min", "3", "-filter_hits", "2", "-filter_frac", "0.25",
                             "-filter_keep", "matched"])
    assert (args.filter_min, args.filter_hits, args.filter_frac, args.filter_keep) == (3, 2, 0.25, "matched")
    for frac in ("0", "1", "1.0", "1e-6"):
        assert cli.parseargs(["-i", fasta, "-k", "5", "-filter", fasta, "-filter_frac", frac])[0].filter_frac == float(frac)
    for name, kind in (("x.faa.gz", "protein"), ("x.fastq.gz", "nucleotide"), ("x.fq", "nucleotide"), ("x.fna", "nucleotide")):
        (tmp_path / name).write_bytes(b"")
        assert cli.parseargs(["-i", fasta, "-k", "5", "-filter", str(tmp_path / name)])[0].filter_kind == kind
    args, _ = cli.parseargs(["-i", fasta, "-k", "5"])
    assert args.filter is None and args.filter_kind is None


def test_cli_rejects(tmp_path, capsys):
    fasta = str(GOLDEN / "inputs" / "A.fasta")
    out = tmp_path / "out"
    bad = [["-filter", str(tmp_path / "missing.fa")], ["-filter", str(ROOT / "README.md")],
           ["-filter", fasta, "-filter_min", "0"], ["-filter", fasta, "-filter_min", "-3"], ["-filter", fasta, "-filter_min", "x"],
           ["-filter", fasta, "-filter_min", str(1 << 64)],
           ["-filter", fasta, "-filter_hits", "0"], ["-filter", fasta, "-filter_hits", "-1"], ["-filter", fasta, "-filter_hits", "1.5"],
           ["-filter", fasta, "-filter_frac", "-0.1"], ["-filter", fasta, "-filter_frac", "1.01"], ["-filter", fasta, "-filter_frac", "nan"],
           ["-filter", fasta, "-filter_frac", "half"],
           ["-filter", fasta, "-filter_keep", "both"], ["-filter", fasta, "-filter_keep", ""],
           ["-filter_min", "2"], ["-filter_hits", "2"], ["-filter_frac", "0.5"], ["-filter_keep", "matched"], ["-filter_min", "1"]]
    for extra in bad:
        with pytest.raises(SystemExit) as e:
            cli.main(["-i", fasta, "-k", "5", "-o", str(out)] + extra)
        assert e.value.code == 2 and not out.exists(), extra  # (before the output folder is made, before any counting)
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        cli.parseargs(["-h"])
    text = " ".join(capsys.readouterr().out.split())
    assert e.value.code == 0 and "-filter FILE" in text and "so the output is FASTA" in text and "{matched,unmatched}" in text
