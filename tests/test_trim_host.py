"""Host-side checks of the trim calls (mk_trim_text / mk_trim_device): the rule's hand examples against its plain-Python
restatement (tests/trim_rule.py), header, binding, report format and CLI layers.  No kernel is launched here;
tests/test_gpu_trim.py trims on the GPU."""
import ctypes as C
import re

import numpy as np
import pytest

import trim_rule
from conftest import GOLDEN, ROOT
from mercat2_amd import cli, kmers, native, report

HEADER = (ROOT / "include" / "mercat_hip.h").read_text()
CTYPE = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int32_t": C.c_int32, "double": C.c_double}
HAND_TABLE = {"ACG": 2, "CGT": 2, "GTA": 1, "TAC": 2}


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


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("text,out,kept", [
    (b">r x\nACGTAC\n", b">r x\nACGT\n", [4]),
    (b">q\nGTACG\n", b"", [0]),
    (b">s\nACGT\n", b">s\nACGT\n", [4]),
    (b">t\nAC\n", b"", [0]),
    (b">w\r\nAC\r\nGT*AC\r\n", b">w\r\nACGT\n", [4]),
])
def test_hand_examples(text, out, kept):
    assert trim_rule.expected(text, HAND_TABLE, 3, 2) == (out, kept)


def test_rule_details():
    # records in one text, a headless start, a lone CR behind a header, a header line with leading blanks, no last newline
    text = b"ACGT\n>r x\nACGTAC\n  >b\rAC\rGT\r>q\nGTACG\n>h\n>e\n\n>last\nACG"
    out, kept = trim_rule.expected(text, HAND_TABLE, 3, 2)
    assert kept == [4, 4, 4, 0, 0, 0, 3] and out == b"ACGT\n>r x\nACGT\n  >b\rACGT\n>last\nACG\n"
    assert len(out) <= len(text) + 1
    # min_len above what is left drops the record; min_len 0 means k
    assert trim_rule.expected(text, HAND_TABLE, 3, 2, min_len=4)[1] == [4, 4, 4, 0, 0, 0, 0]
    assert trim_rule.expected(b">a\nACGTA\n", HAND_TABLE, 3, 2, min_len=5) == (b"", [0])
    # at_least 1: only an absent k-mer is low; the identity on one-line LF records
    whole = b">r x\nACGTAC\n>s\nACGT\n"
    assert trim_rule.expected(whole, HAND_TABLE, 3, 1) == (whole, [6, 4])
    assert trim_rule.expected(b">r\nACGTACC\n", HAND_TABLE, 3, 1) == (b">r\nACGTAC\n", [6])
    # fold: a window counts under min(window, reverse complement)
    assert trim_rule.expected(b">f\nCGTA\n", {"ACG": 2, "GTA": 2, "TAC": 2}, 3, 2, fold=True)[1] == [4]  # CGT -> ACG, GTA stays
    assert trim_rule.expected(b">f\nCGTA\n", {"ACG": 2, "GTA": 2, "TAC": 2}, 3, 2)[1] == [0]


# ---------------------------------------------------------------------------------------------- the header
def test_header_declares_the_calls_and_flags():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ("mk_trim_text", "mk_trim_device"):
        assert re.search(r"\bint %s\s*\(mk_ctx\*" % name, code)
        assert name in native.ABI_SYMBOLS and getattr(native.lib(), name) is not None
    assert re.search(r"#define MK_TRIM_FOLD\s+1u", code)
    assert native.TRIM_FOLD == native.SCREEN_FOLD == 1
    args = re.search(r"int mk_trim_text\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "ctx", "text", "n", "piece_bytes", "flags", "rule", "out", "out_cap", "out_len", "kept", "rows", "cap", "nrows", "st"]
    args = re.search(r"int mk_trim_device\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "ctx", "d_text", "n", "flags", "rule", "d_out", "out_cap", "out_len", "d_kept", "d_rows", "cap", "nrows", "st"]
    assert len(native.lib().mk_trim_text.argtypes) == 14 and len(native.lib().mk_trim_device.argtypes) == 13
    # the trim block follows the track block and stands in front of the merged export
    assert code.index("mk_track_device") < code.index("MK_TRIM_FOLD") < code.index("mk_trim_rule_t") < code.index("mk_trim_text") \
        < code.index("mk_trim_device") < code.index("mk_merged_export")
    # the older call of that stem is still what it was
    assert re.search(r"\bint mk_trim\(mk_ctx\* ctx\);", code) and "mk_trim" in native.ABI_SYMBOLS


def test_bound_structs_match_the_header():
    want_size, _, want = _layout("mk_trim_t")
    assert [f for f, _ in want] == [g[0] for g in native.Trim._fields_]
    assert [(f, getattr(native.Trim, f).offset) for f, _ in want] == want
    assert C.sizeof(native.Trim) == want_size == 96 + 7 * 8 + 4 * 8 == 184
    for (ctype, field), (_, got) in zip(_struct_fields("mk_trim_t"), native.Trim._fields_):
        assert got is (native.Screen if ctype == "mk_screen_t" else CTYPE[ctype]), field
    assert _struct_fields("mk_trim_t")[0] == ("mk_screen_t", "screen") and native.Trim.screen.offset == 0
    assert [f for _, f in _struct_fields("mk_trim_t")[1:]] == [
        "records_out", "records_trimmed", "records_dropped", "bases_in", "bases_out", "bytes_out", "preamble",
        "s_place", "s_first", "s_gather", "s_write"]
    want_size, _, want = _layout("mk_trim_rule_t")
    assert want == [("at_least", 0), ("min_len", 8)] and C.sizeof(native.TrimRule) == want_size == 16
    assert [(f, getattr(native.TrimRule, f).offset) for f, _ in native.TrimRule._fields_] == want
    st = native.Trim()
    st.screen.records, st.records_out, st.records_trimmed, st.bases_out, st.s_first = 7, 5, 3, 99, 0.5
    d = st.as_dict()
    assert d["records"] == 7 and d["records_out"] == 5 and d["records_trimmed"] == 3 and d["bases_out"] == 99 and d["s_first"] == 0.5
    assert {"records_dropped", "bases_in", "bytes_out", "preamble", "s_place", "s_gather", "s_write", "s_probe", "pieces"} <= set(d)


def test_the_abi_number_stands():
    assert native.MK_ABI == 6 and native.lib().mk_version().decode().split()[1].split(".")[0] == "6"


def test_python_layers_are_there():
    for name in ("trim", "trim_device"):
        assert callable(getattr(native.Counter, name))
    assert callable(kmers.trim_reads) and "FASTQ" in kmers.trim_reads.__doc__ and "fq2fa" in kmers.trim_reads.__doc__
    assert callable(report.write_trim_tsv)
    import inspect
    assert list(inspect.signature(native.Counter.trim).parameters)[1:] == ["path_or_bytes", "at_least", "min_len", "fold", "piece_bytes", "info"]
    assert inspect.signature(native.Counter.trim).parameters["at_least"].default == 2
    assert list(inspect.signature(kmers.trim_reads).parameters)[:5] == ["table", "file", "out_path", "at_least", "min_len"]


def test_record_lengths_number_the_records_as_the_names_do():
    text = b"ACGT\n>r x\nAC*GT\r\n AC \n  >b\rAC\rGT\r>h\n>e\n\n>last\nACG"
    assert kmers.record_names(text) == ["", "r", "b", "h", "e", "last"]
    assert kmers.record_lengths(text) == [4, 6, 4, 0, 0, 3] == [len(seq) for _, seq in trim_rule.records(text)]
    assert kmers.record_lengths(b"\n \n>a\nAC\n") == [2] and kmers.record_lengths(b"") == []


# ----------------------------------------------------------------------------------------------- the report
def test_trim_tsv_format(tmp_path):
    names = ["r1", "", "gone"]
    lengths = [150, 18446744073709551615, 20]
    kept = np.array([97, 18446744073709551615, 0], dtype=np.uint64)
    want = b"record\tlength\tkept\nr1\t150\t97\n\t18446744073709551615\t18446744073709551615\ngone\t20\t0\n"
    assert report.write_trim_tsv(tmp_path / "t.tsv", names, lengths, kept) == 3 and (tmp_path / "t.tsv").read_bytes() == want
    assert report.format_trim_tsv([], [], kept[:0]) == b"record\tlength\tkept\n"
    with pytest.raises(ValueError):
        report.write_trim_tsv(tmp_path / "x.tsv", names, lengths, kept[:2])


# -------------------------------------------------------------------------------------------------- the CLI
def test_cli_accepts(tmp_path):
    fasta = str(GOLDEN / "inputs" / "A.fasta")
    args, _ = cli.parseargs(["-i", fasta, "-k", "5", "-trim", fasta])
    assert (args.trim, args.trim_kind, args.trim_min, args.trim_len) == (fasta, "nucleotide", 2, 0)
    args, _ = cli.parseargs(["-i", fasta, "-k", "5", "-trim", fasta, "-trim_min", "3", "-trim_len", "40"])
    assert (args.trim_min, args.trim_len) == (3, 40)
    for name, kind in (("x.faa.gz", "protein"), ("x.fastq.gz", "nucleotide"), ("x.fq", "nucleotide"), ("x.fna", "nucleotide")):
        (tmp_path / name).write_bytes(b"")
        assert cli.parseargs(["-i", fasta, "-k", "5", "-trim", str(tmp_path / name)])[0].trim_kind == kind
    args, _ = cli.parseargs(["-i", fasta, "-k", "5"])
    assert args.trim is None and args.trim_kind is None and args.trim_min is None and args.trim_len is None


def test_cli_rejects(tmp_path, capsys):
    fasta = str(GOLDEN / "inputs" / "A.fasta")
    out = tmp_path / "out"
    for extra in (["-trim", str(tmp_path / "missing.fa")], ["-trim", str(ROOT / "README.md")], ["-trim_min", "2"], ["-trim_len", "30"],
                  ["-trim", fasta, "-trim_min", "0"], ["-trim", fasta, "-trim_min", "-1"], ["-trim", fasta, "-trim_len", "0"],
                  ["-trim", fasta, "-trim_min", "x"]):
        with pytest.raises(SystemExit) as e:
            cli.main(["-i", fasta, "-k", "5", "-o", str(out)] + extra)
        assert e.value.code == 2 and not out.exists(), extra  # (before the output folder is made, before any counting)
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        cli.parseargs(["-h"])
    text = " ".join(capsys.readouterr().out.split())
    assert e.value.code == 0 and "-trim FILE" in text and "-trim_min" in text and "-trim_len" in text and "_trimmed.fna" in text
