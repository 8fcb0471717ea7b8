"""mk_fastq_qc_* without a GPU: the rule of tests/qc_rule.py on hand examples whose tables are written out, the percentile
and mean rule of the writers, the TSV writers byte for byte, the header, the bindings and the command line's refusals."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import qc_rule as rule
from conftest import ROOT
from mercat2_amd import cli, kmers, native, report

HEADER = (ROOT / "include" / "mercat_hip.h").read_text()


def fq(*reads, base=33):
    return b"".join(b"@r%d\n" % i + seq + b"\n+\n" + bytes(v + base for v in q) + b"\n" for i, (seq, q) in enumerate(reads))


def nonzero(table):
    """{index tuple: count} of a table's nonzero entries."""
    return {tuple(int(i) for i in idx): int(table[tuple(idx)]) for idx in np.argwhere(table)}


# ------------------------------------------------------------------------------------------------ hand examples
def test_three_records_by_hand():
    text = fq((b"ACGT", [30, 30, 20, 10]), (b"GGn", [40, 2, 2]), (b"cU", [0, 41]))
    got = rule.run(text, max_pos=4)
    assert {k: got[k].shape for k in rule.TABLES} == {"pos_qual": (1, 5, 96), "pos_base": (1, 5, 8), "read_len": (1, 6),
                                                      "read_qual": (1, 96), "read_gc": (1, 101)}
    assert nonzero(got["pos_qual"]) == {(0, 0, 30): 1, (0, 0, 40): 1, (0, 0, 0): 1, (0, 1, 30): 1, (0, 1, 2): 1, (0, 1, 41): 1,
                                        (0, 2, 20): 1, (0, 2, 2): 1, (0, 3, 10): 1}
    assert nonzero(got["pos_base"]) == {(0, 0, 0): 1, (0, 0, 2): 1, (0, 0, 1): 1, (0, 1, 1): 1, (0, 1, 2): 1, (0, 1, 5): 1,
                                        (0, 2, 2): 1, (0, 2, 4): 1, (0, 3, 3): 1}
    assert nonzero(got["read_len"]) == {(0, 4): 1, (0, 3): 1, (0, 2): 1}
    # means 90 // 4, 44 // 3, 41 // 2; GC 2 of 4, 2 of 3 (66.67 -> 67), 1 of 2
    assert nonzero(got["read_qual"]) == {(0, 22): 1, (0, 14): 1, (0, 20): 1}
    assert nonzero(got["read_gc"]) == {(0, 50): 2, (0, 67): 1}
    assert got["rows"].tolist() == [[4, 90, 2, 0], [3, 44, 2, 1], [2, 41, 1, 0]]
    assert got["figures"] == dict(records=3, lines=12, bases=9, min_len=[2, 0], max_len=[4, 0])
    # the same reads as one pair and a half: refused; as two pairs: the classes alternate
    with pytest.raises(rule.QcError) as e:
        rule.run(text, paired=1)
    assert e.value.code == rule.ERR_RANGE
    pairs = rule.run(text + fq((b"", [])), max_pos=4, paired=1)
    assert nonzero(pairs["read_len"]) == {(0, 4): 1, (0, 2): 1, (1, 3): 1, (1, 0): 1}
    assert nonzero(pairs["read_gc"]) == {(0, 50): 2, (1, 67): 1} and pairs["pos_qual"][1].sum() == 3
    assert pairs["figures"]["min_len"] == [2, 0] and pairs["figures"]["max_len"] == [4, 3]


def test_an_empty_read_counts_only_as_a_length():
    got = rule.run(fq((b"", []), (b"A", [7])))
    assert nonzero(got["read_len"]) == {(0, 0): 1, (0, 1): 1}
    assert nonzero(got["read_qual"]) == {(0, 7): 1} and nonzero(got["read_gc"]) == {(0, 0): 1}
    assert got["rows"].tolist() == [[0, 0, 0, 0], [1, 7, 0, 0]] and got["pos_qual"].sum() == 1
    assert rule.run(b"")["figures"] == dict(records=0, lines=0, bases=0, min_len=[0, 0], max_len=[0, 0])
    assert rule.run(b"\n\n")["read_len"].sum() == 0


def test_the_clip_at_95():
    got = rule.run(fq((b"AAAA", [94, 95, 96, 222])))
    assert nonzero(got["pos_qual"]) == {(0, 0, 94): 1, (0, 1, 95): 1, (0, 2, 95): 1, (0, 3, 95): 1}
    assert got["rows"].tolist() == [[4, 507, 0, 0]]  # (qsum is not clipped)
    assert nonzero(got["read_qual"]) == {(0, 95): 1}  # 507 // 4 = 126
    assert nonzero(rule.run(fq((b"AA", [95, 96])))["read_qual"]) == {(0, 95): 1}
    assert nonzero(rule.run(fq((b"AA", [94, 95])))["read_qual"]) == {(0, 94): 1}


def test_gc_rounds_half_up():
    reads = [(b"GAAAAAAA", [1] * 8),   # 12.5 -> 13
             (b"GCAAAAAA", [1] * 8),   # 25
             (b"GCCAAAAA", [1] * 8),   # 37.5 -> 38
             (b"GAA", [1] * 3),        # 33.33 -> 33
             (b"GGA", [1] * 3),        # 66.67 -> 67
             (b"GC", [1] * 2), (b"NN", [1] * 2)]
    assert nonzero(rule.run(fq(*reads))["read_gc"]) == {(0, 13): 1, (0, 25): 1, (0, 38): 1, (0, 33): 1, (0, 67): 1, (0, 100): 1, (0, 0): 1}


def test_max_pos_smaller_than_the_read():
    got = rule.run(fq((b"ACGTAC", [1, 2, 3, 4, 5, 6]), (b"AC", [9, 9]), (b"ACG", [8, 8, 8])), max_pos=2)
    assert nonzero(got["pos_qual"]) == {(0, 0, 1): 1, (0, 1, 2): 1, (0, 2, 3): 1, (0, 2, 4): 1, (0, 2, 5): 1, (0, 2, 6): 1,
                                        (0, 0, 9): 1, (0, 1, 9): 1, (0, 0, 8): 1, (0, 1, 8): 1, (0, 2, 8): 1}
    assert got["pos_base"][0, 2].tolist() == [1, 1, 2, 1, 0, 0, 0, 0]
    assert got["read_len"].tolist() == [[0, 0, 1, 2]]  # (a read of exactly P bases has its own bin, longer ones share the last)


def test_the_checks_and_the_order_of_the_errors():
    good = fq((b"ACGT", [30] * 4))
    for text, record, kind in ((b">r\nAC\n+\nII\n", 0, "at"), (good + b"@r\nAC\n-\nII\n", 1, "plus"), (good + b"@r\nAC\n+\nIII\n", 1, "length"),
                               (good + b"@r\nAC\n+\nI \n", 1, "qual"), (b">r\nAC\n-\nI \n", 0, "at"), (b"@r\nAC\n+\nI\n@s\nA\n+\n \n", 0, "length"),
                               (good + b"@r\nAC\n", 1, "incomplete"), (good + b"@r\nAC\n+\nI \n@s\n", 1, "qual"),
                               (b"@r\nAC\n+\nI \n" + b">r\nAC\n+\nII\n", 0, "qual")):
        with pytest.raises(rule.QcError) as e:
            rule.run(text)
        assert (e.value.code, e.value.record, e.value.kind) == (rule.ERR_UNSUPPORTED, record, kind)
    with pytest.raises(rule.QcError) as e:  # 'I' is a quality from '@' up, '?' is not
        rule.run(b"@r\nAC\n+\nI?\n", phred_base=64)
    assert e.value.kind == "qual"
    assert rule.run(b"@r\nAC\n+\nI@\n", phred_base=64)["rows"].tolist() == [[2, 9, 1, 0]]
    assert rule.run(good + b"\n\n\n")["figures"]["lines"] == 7
    assert rule.run(b"@a x\r\nACGT\r\n+a\r\nIIII\r\n@b\nAC\n+\nII")["rows"].tolist() == [[4, 160, 2, 0], [2, 80, 1, 0]]
    for bad in (dict(phred_base=34), dict(max_pos=0), dict(max_pos=16385), dict(paired=2)):
        with pytest.raises(rule.QcError) as e:
            rule.run(good, **bad)
        assert e.value.code == rule.ERR_ARG
    with pytest.raises(rule.QcError) as e:
        rule.run(good * 3, cap=2)
    assert e.value.code == rule.ERR_RANGE and e.value.counts == (3, 2)
    assert rule.run(good * 3, cap=None)["figures"]["records"] == 3


# ------------------------------------------------------------------------------------------------- the writers
def test_percentiles_and_mean_on_hand_histograms():
    hist = [0] * 96
    hist[10], hist[20], hist[30] = 1, 8, 1  # cum 1, 9, 10 of 10
    assert [report.qc_percentile(hist, x) for x in (10, 25, 50, 75, 90)] == [10, 20, 20, 20, 20]
    assert report.qc_percentile(hist, 91) == 30 and report.qc_percentile(hist, 100) == 30 and report.qc_percentile(hist, 0) == 0
    assert report.qc_mean(hist) == 20.0
    one = [0, 0, 0, 5]
    assert [report.qc_percentile(one, x) for x in (10, 50, 90)] == [3, 3, 3] and report.qc_mean(one) == 3.0
    half = [2, 2]  # exactly half at 0: 100 * 2 >= 50 * 4
    assert report.qc_percentile(half, 50) == 0 and report.qc_percentile(half, 51) == 1 and report.qc_mean(half) == 0.5
    assert report.qc_percentile([0] * 96, 50) == 0 and report.qc_mean([0] * 96) == 0.0


def test_the_tsv_writers_byte_for_byte(tmp_path):
    got = rule.run(fq((b"ACGT", [30, 30, 20, 10]), (b"GGn", [40, 2, 2]), (b"cU", [0, 41]), (b"", [])), max_pos=3)
    assert report.format_qc_cycles(got) == (
        b"mate\tcycle\tbases\tmean\tp10\tq1\tmedian\tq3\tp90\tA\tC\tG\tT\tN\tother\n"
        b"0\t1\t3\t23.33\t0\t0\t30\t40\t40\t1\t1\t1\t0\t0\t0\n"
        b"0\t2\t3\t24.33\t2\t2\t30\t41\t41\t0\t1\t1\t0\t0\t1\n"
        b"0\t3\t2\t11.00\t2\t2\t2\t20\t20\t0\t0\t1\t0\t1\t0\n"
        b"0\t>3\t1\t10.00\t10\t10\t10\t10\t10\t0\t0\t0\t1\t0\t0\n")
    assert report.format_qc_quality(got) == b"mate\tmean_quality\treads\n0\t14\t1\n0\t20\t1\n0\t22\t1\n"
    gc = report.format_qc_gc(got).split(b"\n")
    assert gc[0] == b"mate\tgc\treads" and len(gc) == 103 and gc[-1] == b"" and gc[1] == b"0\t0\t0" and gc[51] == b"0\t50\t2"
    assert gc[68] == b"0\t67\t1" and sum(int(line.split(b"\t")[2]) for line in gc[1:-1]) == 3
    assert report.format_qc_length(got) == b"mate\tlength\treads\n0\t0\t1\n0\t2\t1\n0\t3\t1\n0\t>3\t1\n"
    assert report.format_qc_summary(got) == (
        b"metric\tall\nreads\t4\nbases\t9\nempty_reads\t1\nmin_length\t0\nmean_length\t2.25\nmax_length\t>3\ngc_percent\t55.56\n"
        b"n_bases\t1\nq20_bases\t5\nq30_bases\t4\nmean_quality\t19.44\n")
    paths = report.write_qc_files(tmp_path / "s_raw", got)
    assert [p[len(str(tmp_path)) + 1:] for p in paths] == ["s_raw_cycles.tsv", "s_raw_quality.tsv", "s_raw_gc.tsv", "s_raw_length.tsv",
                                                           "s_raw_summary.tsv"]
    assert open(paths[0], "rb").read() == report.format_qc_cycles(got) and open(paths[4], "rb").read() == report.format_qc_summary(got)
    # two classes: mates 1 and 2, a column each
    pairs = rule.run(fq((b"AC", [30, 30]), (b"G", [10])), max_pos=3, paired=1)
    assert report.format_qc_length(pairs) == b"mate\tlength\treads\n1\t2\t1\n2\t1\t1\n"
    assert report.format_qc_cycles(pairs).split(b"\n")[1:4] == [b"1\t1\t1\t30.00\t30\t30\t30\t30\t30\t1\t0\t0\t0\t0\t0",
                                                                b"1\t2\t1\t30.00\t30\t30\t30\t30\t30\t0\t1\t0\t0\t0\t0",
                                                                b"2\t1\t1\t10.00\t10\t10\t10\t10\t10\t0\t0\t1\t0\t0\t0"]
    assert report.format_qc_summary(pairs).split(b"\n")[:3] == [b"metric\tmate1\tmate2", b"reads\t1\t1", b"bases\t2\t1"]
    assert report.format_qc_summary(rule.run(b"")).split(b"\n")[1:7] == [b"reads\t0", b"bases\t0", b"empty_reads\t0", b"min_length\t0",
                                                                        b"mean_length\t0.00", b"max_length\t0"]


# ----------------------------------------------------------------------------------------- header and bindings
CTYPE = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double, "uint64_t*": C.c_void_p}


def _struct_fields(name):
    """[(C type, field, array length or 0)] of a struct of the header."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if stmt:
            ctype, rest = stmt.split(" ", 1)
            for f in rest.split(","):
                m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", f.strip())
                out.append((ctype, m.group(1), int(m.group(2) or 0)))
    return out


def test_header_declares_the_calls_and_the_version_stands():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ("mk_fastq_qc_text", "mk_fastq_qc_device"):
        assert name in native.ABI_SYMBOLS and getattr(native.lib(), name) is not None
    args = re.search(r"int mk_fastq_qc_text\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["ctx", "fastq", "n", "piece_bytes", "opt", "cap", "out", "nrec", "st"]
    args = re.search(r"int mk_fastq_qc_device\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["ctx", "d_fastq", "n", "opt", "cap", "d_out", "nrec", "st"]
    assert len(native.lib().mk_fastq_qc_text.argtypes) == 9 and len(native.lib().mk_fastq_qc_device.argtypes) == 8
    assert re.search(r"#define MK_QC_MAX_POS 16384\b", code) and re.search(r"#define MK_QC_QBINS 96\b", code)
    assert (native.QC_MAX_POS, native.QC_QBINS, native.QC_GC_BINS) == (16384, 96, 101) == (rule.MAX_POS, rule.QBINS, rule.GC_BINS)
    rule_text = " ".join(HEADER.split("per-cycle quality control of a FASTQ text")[1].split("#define MK_QC_MAX_POS")[0].replace(" * ", " ").split())
    for phrase in ("its quality line holds a character below the phred base", "row P collects every cycle from P on",
                   "g = (200 gc + L) / (2 L)", "m = min(qsum / L, 95)", "columns 6 and 7 stay 0", "not when rows is NULL",
                   "at most 2^32 - 1 bytes", "aligned to 8", "nothing depends on piece_bytes", "an odd record count is MK_ERR_RANGE"):
        assert phrase in rule_text, phrase
    assert native.MK_ABI == 6 and native.lib().mk_version().decode() == "mercat_hip 6.1 (gfx950)"


def test_bound_structs_match_the_header():
    fields = _struct_fields("mk_qc_opt_t")
    assert [(CTYPE[t], f) for t, f, _ in fields] == [(t, f) for f, t in native.QcOpt._fields_] and C.sizeof(native.QcOpt) == 12
    assert [f for _, f, _ in fields] == ["phred_base", "max_pos", "paired"]
    fields = _struct_fields("mk_qc_out_t")
    assert [f for _, f, _ in fields] == ["pos_qual", "pos_base", "read_len", "read_qual", "read_gc", "rows"] == list(native.QC_TABLES) + ["rows"]
    assert [(CTYPE[t], f) for t, f, _ in fields] == [(t, f) for f, t in native.QcOut._fields_] and C.sizeof(native.QcOut) == 48
    fields = _struct_fields("mk_fastq_qc_t")
    assert [(f, n) for _, f, n in fields] == [("records", 0), ("lines", 0), ("bases", 0), ("min_len", 2), ("max_len", 2), ("s_copy", 0),
                                              ("s_index", 0), ("s_reads", 0), ("s_cycles", 0), ("s_write", 0)]
    assert [(CTYPE[t] * n if n else CTYPE[t], f) for t, f, n in fields] == [(t, f) for f, t in native.FastqQc._fields_]
    assert [getattr(native.FastqQc, f).offset for _, f, _ in fields] == [0, 8, 16, 24, 40, 56, 64, 72, 80, 88] and C.sizeof(native.FastqQc) == 96
    st = native.FastqQc()
    st.bases, st.s_cycles = 3, 0.5
    st.max_len[1] = 7
    assert st.as_dict()["bases"] == 3 and st.as_dict()["s_cycles"] == 0.5 and st.as_dict()["max_len"] == [0, 7]
    assert set(st.as_dict()) == {f for _, f, _ in fields}


def test_python_layers_are_there():
    assert list(inspect.signature(native.Counter.fastq_qc).parameters)[1:] == ["path_or_bytes", "max_pos", "phred_base", "paired", "rows",
                                                                              "piece_bytes", "info"]
    d = {k: p.default for k, p in inspect.signature(native.Counter.fastq_qc).parameters.items()}
    assert (d["max_pos"], d["phred_base"], d["paired"], d["rows"], d["piece_bytes"], d["info"]) == (512, 33, False, False, 0, None)
    assert callable(native.Counter.fastq_qc_device)
    opt = native.qc_options(max_pos=150, phred_base=64, paired=True)
    assert (opt.max_pos, opt.phred_base, opt.paired) == (150, 64, 1)
    for bad in (dict(max_pos=-1), dict(phred_base=1 << 32)):
        with pytest.raises(ValueError):
            native.qc_options(**bad)
    assert native.qc_shapes(150, True) == rule.shapes(150, 1) and native.qc_shapes(1, False) == rule.shapes(1, 0)
    assert native.QC_COLUMNS == ("length", "qsum", "gc", "n") and native.QC_BASES == ("A", "C", "G", "T", "N", "other")
    names = list(inspect.signature(kmers.qc_reads).parameters)
    assert names == ["file", "out_prefix", "max_pos", "phred_base", "paired", "mate_file", "device"]
    d = {k: p.default for k, p in inspect.signature(kmers.qc_reads).parameters.items()}
    assert (d["out_prefix"], d["max_pos"], d["phred_base"], d["paired"], d["mate_file"], d["device"]) == (None, 512, 33, False, None, 0)
    assert "not fastqc's" in kmers.qc_reads.__doc__
    with pytest.raises(ValueError):  # (before any call of the library)
        kmers.qc_reads("reads.fna")
    assert set(report.QC_FILES) == {"cycles", "quality", "gc", "length", "summary"}


# ------------------------------------------------------------------------------------------------ the command line
@pytest.fixture()
def files(tmp_path):
    (tmp_path / "s.fna").write_bytes(b">a\nACGTACGTAC\n")
    (tmp_path / "r.fastq").write_bytes(b"@a\nACGTACGTAC\n+\nIIIIIIIIII\n")
    (tmp_path / "dir").mkdir()
    (tmp_path / "dir" / "t.fq").write_bytes(b"@a\nACGTACGTAC\n+\nIIIIIIIIII\n")
    return tmp_path


def parse(files, inputs, *extra):
    return cli.parseargs(list(inputs) + ["-k", "5", "-o", str(files / "out")] + [str(x) for x in extra])[0]


def test_cli_accepts_qc(files):
    args = parse(files, ["-i", str(files / "r.fastq")], "-qc", "-skipclean")
    assert args.qc == 512 and args.qc_phred is None and args.qc_paired is False
    args = parse(files, ["-i", str(files / "s.fna"), str(files / "r.fastq")], "-qc", 150, "-qc_phred", 64, "-qc_paired", "-qtrim", 20)
    assert (args.qc, args.qc_phred, args.qc_paired, args.qtrim) == (150, 64, True, 20)
    assert parse(files, ["-f", str(files / "dir")], "-qc", 16384, "-skipclean").qc == 16384
    assert parse(files, ["-i", str(files / "r.fastq")], "-skipclean").qc is None


def test_the_help_says_what_qc_is_not(capsys):
    with pytest.raises(SystemExit) as e:
        cli.parseargs(["-h"])
    help_ = " ".join(capsys.readouterr().out.split())
    assert e.value.code == 0 and "where MerCat2 runs fastqc" in help_ and "not fastqc's" in help_ and "-qc_phred" in help_
    assert "-qc [MAXPOS]" in " ".join(cli.__doc__.split()) and "mk_fastq_qc_text" in cli.__doc__


@pytest.mark.parametrize("extra,message", [
    (["-qc_phred", 64], "-qc_phred needs -qc"),
    (["-qc_paired"], "-qc_paired needs -qc"),
    (["-qc", 0], "-qc 0: must lie in 1..16384"),
    (["-qc", 16385], "-qc 16385: must lie in 1..16384"),
    (["-qc", "-qc_phred", 50], "invalid choice"),
])
def test_cli_refuses(files, capsys, extra, message):
    with pytest.raises(SystemExit) as e:
        parse(files, ["-i", str(files / "r.fastq")], "-skipclean", *extra)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_cli_refuses_qc_without_fastq_input(files, capsys):
    with pytest.raises(SystemExit) as e:
        parse(files, ["-i", str(files / "s.fna")], "-qc")
    assert e.value.code == 2 and "no input is a FASTQ file" in capsys.readouterr().err


def test_qc_does_not_lift_the_refusal_of_untrimmed_fastq(files):
    args = parse(files, ["-i", str(files / "r.fastq")], "-qc")
    assert args.qc == 512 and not args.skipclean and args.qtrim is None
    with pytest.raises(SystemExit) as e:  # (what main() asks of the file with these flags)
        cli.classify(files / "r.fastq", args.skipclean or args.qtrim is not None or args.adapt is not None or args.overlap is not None)
    assert "without -skipclean MerCat2 trims FASTQ reads with fastp" in str(e.value)
