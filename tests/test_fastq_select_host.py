"""Host-side checks of the FASTQ selection (mk_fastq_select_text / mk_fastq_select_device): hand examples of the rule
against its plain-Python restatement (tests/fastq_select_rule.py), the header and the binding, the host routines
mk_fastq_cuts, mk_fq_interleave and mk_fq_split_pairs, and the refusals of the CLI and of kmers.  No kernel is launched
here; tests/test_gpu_fastq_select.py selects on the GPU."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import fastq_select_rule as rule
from conftest import ROOT
from mercat2_amd import cli, kmers, native

HEADER = (ROOT / "include" / "mercat_hip.h").read_text()
CTYPE = {"uint64_t": C.c_uint64, "double": C.c_double}

LF = b"@a x\nACGT\n+\nIIII\n@b\nGG\n+b\n##\n"
CRLF = b"@c\r\nACG\r\n+\r\nIJK\r\n"
OPEN = b"@d\nTTTTT\n+\n12345"


# ------------------------------------------------------------------------------------------------ the rule
def test_lines_and_records():
    assert rule.lines(b"") == [] and rule.lines(b"a") == [b"a"] and rule.lines(b"a\n") == [b"a\n"]
    assert rule.lines(b"a\n\nb") == [b"a\n", b"\n", b"b"] and rule.lines(b"a\r\n") == [b"a\r\n"]
    recs, trailing = rule.records(LF + b"\n\n")
    assert len(recs) == 2 and recs[1] == [b"@b\n", b"GG\n", b"+b\n", b"##\n"] and trailing == [b"\n", b"\n"]
    assert rule.records(b"@\n\n+\n\n") == ([[b"@\n", b"\n", b"+\n", b"\n"]], [])
    assert rule.records(OPEN)[0][0][3] == b"12345"


def test_whole_records_come_back_byte_for_byte():
    assert rule.expected(LF) == LF and rule.expected(CRLF) == CRLF and rule.expected(LF + CRLF) == LF + CRLF
    assert rule.expected(OPEN) == OPEN + b"\n"  # (a last record without its newline gets one)
    assert rule.expected(LF + b"\n\n") == LF    # (trailing empty lines belong to no record)
    assert rule.expected(b"") == b"" and rule.expected(b"\n\n\n") == b""
    assert rule.expected(b"@\n\n+\n\n") == b"@\n\n+\n\n"


def test_keep_and_which():
    text = LF + CRLF + OPEN
    assert rule.expected(text, keep=[1, 0, 1, 0]) == LF[:17] + CRLF
    assert rule.expected(text, keep=[1, 2, 0, 2], which=2) == LF[17:] + OPEN + b"\n"
    assert rule.expected(text, keep=[0, 0, 0, 0]) == b""
    assert rule.expected(text, keep=[True, True, True, True]) == text + b"\n"
    for which in (0, 3):
        with pytest.raises(rule.SelectError) as e:
            rule.expected(text, keep=[1, 1, 1, 1], which=which)
        assert e.value.code == rule.ERR_ARG
    assert rule.expected(text, kept=[4, 2, 3, 5], which=7) == rule.expected(text, kept=[4, 2, 3, 5])  # (ignored without keep)


def test_a_trimmed_record():
    assert rule.expected(LF, kept=[2, 2]) == b"@a x\nAC\n+\nII\n@b\nGG\n+b\n##\n"
    assert rule.expected(LF, kept=[4, 0]) == LF[:17] and rule.expected(LF, kept=[4, 2]) == LF
    assert rule.expected(CRLF, kept=[3]) == b"@c\r\nACG\n+\r\nIJK\n"  # (header and plus line as they stand, the cut lines end in LF)
    assert rule.expected(CRLF, kept=[1]) == b"@c\r\nA\n+\r\nI\n"
    assert rule.expected(OPEN, kept=[5]) == OPEN + b"\n" and rule.expected(OPEN, kept=[1]) == b"@d\nT\n+\n1\n"
    assert rule.expected(LF + OPEN, keep=[2, 1, 1], kept=[4, 1, 0]) == b"@b\nG\n+b\n#\n"
    fig = rule.figures(LF + OPEN, keep=[1, 1, 0], kept=[3, 2, 5])
    assert fig == {"records": 3, "records_out": 2, "records_trimmed": 1, "bases_out": 5, "bytes_out": 15 + 12, "lines": 12}
    for text, kept in ((LF, [2, 1]), (CRLF, [2]), (OPEN, [5])):
        assert len(rule.expected(text, kept=kept)) <= len(text) + 1


@pytest.mark.parametrize("text,kept,record,kind", [
    (LF + b">e\nAC\n+\nII\n", None, 2, "at"),
    (LF + b"\n@e\nAC\n+\nII\n", None, 2, "at"),               # (an empty line shifts every record behind it)
    (b"@e\nAC\n-\nII\n" + LF, None, 0, "plus"),
    (LF + b"@e\nAC\n\nII\n", None, 2, "plus"),
    (LF + b"@e\nACG\n+\nII\n", None, 2, "length"),
    (LF + b"@e\nAC\r\n+\nII\r\r\n", None, 2, "length"),       # (one trailing CR is not counted, a second is)
    (b"@e\nA C\n+\nIII\n", [1], 0, "blank"),
    (b"@e\nA*C\n+\nIII\n", [1], 0, "blank"),
    (b"@e\nAC\t\n+\nIII\n", [1], 0, "blank"),
    (b"@e\nA\rC\n+\nIII\n", [1], 0, "blank"),
    (LF + b"@e\nA\x1cC\n+\nIII\n", [1, 1, 1], 2, "blank"),
    (LF, [4, 3], 1, "kept"),
    (LF + b"@e\nAC\n", None, 2, "incomplete"),
    (LF + b"@e", None, 2, "incomplete"),
    (LF + b"\n\nx", None, 2, "incomplete"),
    (LF + b"\n\n\nx", None, 2, "at"),                         # (four lines are a record, however empty)
    (b"@e\nAC\n-\nI\n" + b"@f\nAC\n", None, 0, "plus"),       # (the lowest record wins)
    (b">e\nAC\n-\nI\n", None, 0, "at"),                        # (and its first check)
])
def test_each_malformed_kind_names_its_record(text, kept, record, kind):
    assert rule.check(text, kept is not None, kept) == (record, kind)
    with pytest.raises(rule.SelectError) as e:
        rule.expected(text, kept=kept)
    assert (e.value.record, e.value.kind) == (record, kind)
    assert e.value.code == (rule.ERR_RANGE if kind == "kept" else rule.ERR_UNSUPPORTED) and kind in rule.PHRASE


def test_blanks_only_matter_when_kept_is_given():
    text = b"@e\nA C*\n+\nIIII\n"
    assert rule.expected(text) == text and rule.expected(text, keep=[1]) == text
    assert rule.check(b"@e\nAC\r\n+\nII\n", True) is None  # (the CR of CR LF is no blank)


def test_record_count_mismatch():
    for keep in ([1], [1, 1, 1]):
        with pytest.raises(rule.SelectError) as e:
            rule.expected(LF, keep=keep)
        assert e.value.code == rule.ERR_RANGE and e.value.counts == (2, len(keep))
    with pytest.raises(rule.SelectError) as e:  # (the count is checked before the records are)
        rule.expected(b">x\nA\n+\nI\n", nrec=2)
    assert e.value.code == rule.ERR_RANGE and e.value.counts == (1, 2)


# ---------------------------------------------------------------------------------------------- the header
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


def test_header_declares_the_calls():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ("mk_fastq_select_text", "mk_fastq_select_device"):
        assert re.search(r"\bint %s\s*\(mk_ctx\*" % name, code)
    for name in ("mk_fastq_select_text", "mk_fastq_select_device", "mk_fastq_cuts", "mk_fq_interleave", "mk_fq_split_pairs"):
        assert name in native.ABI_SYMBOLS and getattr(native.lib(), name) is not None
    args = re.search(r"int mk_fastq_select_text\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "ctx", "fastq", "n", "piece_bytes", "keep", "kept", "nrec", "which", "out", "out_cap", "out_len", "st"]
    args = re.search(r"int mk_fastq_select_device\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "ctx", "d_fastq", "n", "d_keep", "d_kept", "nrec", "which", "d_out", "out_cap", "out_len", "st"]
    assert len(native.lib().mk_fastq_select_text.argtypes) == 12 and len(native.lib().mk_fastq_select_device.argtypes) == 11
    args = re.search(r"int mk_fastq_cuts\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["text", "n", "piece", "cuts", "cap", "ncuts"]
    # the comment of the error code speaks of the new use, and the ABI number stands: nothing older changed
    assert "mk_fastq_select_" in re.search(r"#define MK_ERR_UNSUPPORTED.*?\*/", HEADER, re.S).group(0)
    assert native.MK_ABI == 6 and native.lib().mk_version().decode().split()[1].split(".")[0] == "6"


def test_bound_struct_matches_the_header():
    fields = _struct_fields("mk_fastq_select_t")
    assert [f for _, f in fields] == ["records", "records_out", "records_trimmed", "bases_out", "bytes_out", "lines",
                                      "s_copy", "s_index", "s_place", "s_gather", "s_write"]
    assert [f for _, f in fields] == [g[0] for g in native.FastqSelect._fields_]
    for (ctype, field), (_, got) in zip(fields, native.FastqSelect._fields_):
        assert got is CTYPE[ctype], field
    assert [getattr(native.FastqSelect, f).offset for _, f in fields] == [8 * i for i in range(11)]
    assert C.sizeof(native.FastqSelect) == 6 * 8 + 5 * 8 == 88
    st = native.FastqSelect()
    st.records, st.records_trimmed, st.lines, st.s_gather = 9, 4, 36, 0.25
    assert st.as_dict()["records"] == 9 and st.as_dict()["records_trimmed"] == 4 and st.as_dict()["lines"] == 36 and \
        st.as_dict()["s_gather"] == 0.25 and set(st.as_dict()) == {f for _, f in fields}


def test_python_layers_are_there():
    assert list(inspect.signature(native.Counter.fastq_select).parameters)[1:] == [
        "path_or_bytes", "keep", "kept", "which", "piece_bytes", "info"]
    assert inspect.signature(native.Counter.fastq_select).parameters["which"].default == 1
    assert callable(native.Counter.fastq_select_device)
    for fn in (kmers.filter_reads, kmers.trim_reads, kmers.normalize_read_pairs):
        p = inspect.signature(fn).parameters["fastq_out"]
        assert p.default is False and list(inspect.signature(fn).parameters)[-1] == "fastq_out"
        assert "thrown away" in fn.__doc__
    # normalize_reads keeps the arguments it has (its own tests pin them): its FASTQ form is a function beside it
    assert list(inspect.signature(kmers.normalize_reads_fastq).parameters) == list(inspect.signature(kmers.normalize_reads).parameters)
    assert "thrown away" in kmers.normalize_reads_fastq.__doc__ and "normalize_reads_fastq" in kmers.normalize_reads.__doc__
    with pytest.raises(ValueError):  # (before any call of the library)
        native._select_arrays([1, 0, 1], [5, 5])
    keep, kept, n = native._select_arrays([True, False], [7, 0])
    assert keep.dtype == np.uint8 and kept.dtype == np.uint64 and n == 2 and keep.tolist() == [1, 0]
    assert native._select_arrays(None, None)[2] == -1


# ------------------------------------------------------------------------------------------- mk_fastq_cuts
def _fastq(rng, reads, crlf=False, final_newline=True):
    nl = b"\r\n" if crlf else b"\n"
    out = []
    for i in range(reads):
        n = int(rng.integers(0, 40))
        seq = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))
        qual = bytes(rng.integers(33, 74, n, dtype=np.uint8))
        out.append(b"@r%d" % i + nl + seq + nl + b"+" + nl + qual + nl)
    text = b"".join(out)
    return text if final_newline else text[:-len(nl)]


@pytest.mark.parametrize("crlf,final_newline", [(False, True), (True, True), (False, False), (True, False)])
def test_cuts_fall_only_behind_lines_4j(crlf, final_newline):
    rng = np.random.default_rng(11)
    text = _fastq(rng, 60, crlf, final_newline)
    starts = np.cumsum([0] + [len(line) for line in rule.lines(text)]).tolist()
    for piece in (1, 7, 64, 300, len(text), len(text) + 5):
        got = native.fastq_cuts(text, piece).tolist()
        assert got == rule.cuts(text, piece), piece
        assert all(c in starts[4::4] and 0 < c < len(text) for c in got)
        ends = [0] + got + [len(text)]
        assert all(b - a >= piece for a, b in zip(ends[:-2], ends[1:-1]))  # (every piece but the last holds `piece` bytes)
    assert len(native.fastq_cuts(text, 1)) == 59  # (piece smaller than a record: a record a piece)
    assert native.fastq_cuts(text, len(text) + 5).tolist() == []


def test_cuts_of_small_texts():
    for text in (b"", b"\n", b"@\n\n+\n\n", b"@\n\n+\n", b"@\n\n+\n\n\n", b"@\n\n+\n\n@"):
        assert native.fastq_cuts(text, 1).tolist() == rule.cuts(text, 1), text
    assert native.fastq_cuts(b"@\n\n+\n\n\n", 1).tolist() == [6] and native.fastq_cuts(b"@\n\n+\n\n@\n\n+\n\n", 1).tolist() == [6]
    # cap too small: the needed size comes back
    cuts, need = np.zeros(1, np.uint64), C.c_size_t(0)
    text = b"@\n\n+\n\n" * 5
    assert native.lib().mk_fastq_cuts(text, len(text), 1, cuts.ctypes.data, 1, C.byref(need)) == -7 and need.value == 4


# ------------------------------------------------------------------- mk_fq_interleave / mk_fq_split_pairs
def test_interleave_and_split_round_trip():
    rng = np.random.default_rng(12)
    a, b = _fastq(rng, 25), _fastq(rng, 25, crlf=True)
    both = native.interleave_fastq(a, b)
    assert both == rule.interleave(a, b) and len(both) == len(a) + len(b)
    assert native.split_pairs_fastq(both) == (a, b) == rule.split(both)
    assert native.interleave_fastq(b"", b"") == b"" and native.split_pairs_fastq(b"") == (b"", b"")
    assert native.interleave_fastq(a + b"\n\n", b) == both  # (empty lines behind the last record are dropped)


def test_interleave_gives_a_last_record_its_newline():
    a, b = b"@a\nAC\n+\nII\n@b\nG\n+\nI", b"@c\nTT\n+\n##\n@d\nC\n+\n#"
    both = native.interleave_fastq(a, b)
    assert both == b"@a\nAC\n+\nII\n@c\nTT\n+\n##\n@b\nG\n+\nI\n@d\nC\n+\n#\n" == rule.interleave(a, b)
    assert native.split_pairs_fastq(both[:-1]) == (a + b"\n", b + b"\n") == rule.split(both[:-1])


def test_interleave_and_split_refuse():
    a, b = b"@a\nAC\n+\nII\n@b\nG\n+\nI\n", b"@c\nTT\n+\n##\n"
    with pytest.raises(native.MercatHipError) as e:
        native.interleave_fastq(a, b)
    assert e.value.code == -7 and "2 records" in str(e.value) and "1" in str(e.value)
    with pytest.raises(native.MercatHipError) as e:  # an odd count
        native.split_pairs_fastq(a + b)
    assert e.value.code == -7 and "3 records" in str(e.value)
    with pytest.raises(native.MercatHipError) as e:  # the text ends inside a record
        native.interleave_fastq(a + b"@x\nA\n", a)
    assert e.value.code == -8 and "record 2" in str(e.value)
    with pytest.raises(rule.SelectError):
        rule.interleave(a, b)
    with pytest.raises(rule.SelectError):
        rule.split(a + b)
    # the sizing call, and room one byte short
    need, pairs = C.c_size_t(0), C.c_size_t(0)
    L = native.lib()
    assert L.mk_fq_interleave(a, len(a), a, len(a), None, 0, C.byref(need), C.byref(pairs)) == -7 and need.value == 2 * len(a)
    out = np.full(2 * len(a), 0xEE, np.uint8)
    assert L.mk_fq_interleave(a, len(a), a, len(a), out.ctypes.data, 2 * len(a) - 1, C.byref(need), C.byref(pairs)) == -7
    assert out[-1] == 0xEE and need.value == 2 * len(a)


# --------------------------------------------------------------------------------------------- CLI and kmers
@pytest.fixture()
def files(tmp_path):
    (tmp_path / "s.fna").write_bytes(b">s\nACGTACGTAC\n")
    (tmp_path / "r.fastq").write_bytes(LF)
    (tmp_path / "r2.fq").write_bytes(LF)
    (tmp_path / "r.fna").write_bytes(b">a\nACGT\n")
    (tmp_path / "p.faa").write_bytes(b">p\nMKV\n")
    return tmp_path


def parse(files, *extra):
    return cli.parseargs(["-i", str(files / "s.fna"), "-k", "5", "-skipclean", "-o", str(files / "out")] + [str(x) for x in extra])[0]


def test_cli_accepts_fastq_out(files):
    args = parse(files, "-trim", files / "r.fastq", "-fastq_out")
    assert args.fastq_out and cli.paired_outputs(args, "trim", files, "s_trimmed", "s", "fna") == {
        "out_path": files / "s_trimmed.fastq", "fastq_out": True}
    args = parse(files, "-filter", files / "r.fastq", "-filter_mate", files / "r2.fq", "-filter_keep", "matched", "-singles", "-fastq_out")
    where = cli.paired_outputs(args, "filter", files, "s_matched", "s", "fna")
    assert where["out_path"] == files / "s_matched_1.fastq" and where["out_path2"] == files / "s_matched_2.fastq"
    assert where["singles_path"] == files / "s_singles.fastq" and where["fastq_out"] is True
    args = parse(files, "-norm", files / "r.fastq", "-paired", "-fastq_out")
    assert cli.paired_outputs(args, "norm", files, "s_kept", "s", "fna")["out_path"] == files / "s_kept.fastq"
    args = parse(files, "-trim", files / "r.fastq")  # (without the flag nothing changes)
    assert not args.fastq_out and cli.paired_outputs(args, "trim", files, "s_trimmed", "s", "fna") == {"out_path": files / "s_trimmed.fna"}


@pytest.mark.parametrize("extra,message", [
    (("-fastq_out",), "-fastq_out needs -filter, -trim or -norm FILE"),
    (("-trim", "r.fna", "-fastq_out"), "not a FASTQ file"),
    (("-filter", "r.fna", "-fastq_out"), "not a FASTQ file"),
    (("-norm", "r.fna", "-fastq_out"), "not a FASTQ file"),
    (("-trim", "p.faa", "-fastq_out"), "a protein file has no qualities"),
    (("-trim", "r.fastq", "-correct", "r.fastq", "-fastq_out"), "does not go with -correct"),
])
def test_cli_refuses(files, capsys, extra, message):
    argv = [str(files / x) if "." in x else x for x in extra]
    with pytest.raises(SystemExit) as e:
        parse(files, *argv)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_kmers_refuse_fasta_input(files):
    """fastq_out needs qualities: a '.fna' input is refused before the table is touched (None stands for it here)."""
    out = files / "o.fastq"
    with pytest.raises(ValueError, match="FASTQ"):
        kmers.filter_reads(None, files / "r.fna", out, fastq_out=True)
    with pytest.raises(ValueError, match="FASTQ"):
        kmers.trim_reads(None, files / "r.fna", out, fastq_out=True)
    with pytest.raises(ValueError, match="FASTQ"):
        kmers.normalize_reads_fastq(None, files / "r.fna", out)
    with pytest.raises(ValueError, match="FASTQ"):
        kmers.normalize_read_pairs(None, files / "r.fna", out, fastq_out=True)
    with pytest.raises(ValueError, match="FASTQ"):  # (the mate file too)
        kmers.trim_reads(None, files / "r.fastq", out, mate_file=files / "r.fna", out_path2=files / "o2.fastq", fastq_out=True)
    with pytest.raises(ValueError, match="'@'"):    # (a header line fq2fa would drop)
        (files / "bad.fastq").write_bytes(b">a\nAC\n+\nII\n")
        kmers.trim_reads(None, files / "bad.fastq", out, fastq_out=True)
    assert not out.exists()
