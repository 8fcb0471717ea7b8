"""mk_fastq_dedup_* without a GPU: the rule of tests/dedup_rule.py on a hand example whose result is written out, the TSV
writers byte for byte (the order and tie rule of _overrepresented.tsv included), the header, the bindings and the command
line's refusals."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import dedup_rule as rule
from conftest import ROOT
from mercat2_amd import cli, kmers, native, report

HEADER = (ROOT / "include" / "mercat_hip.h").read_text()
SEQS = [b"ACGTA", b"ACGTA", b"ACGTC", b"ACG", b"", b""]


def fq(seqs, nl=b"\n"):
    return b"".join(b"@r%d" % i + nl + s + nl + b"+" + nl + b"I" * len(s) + nl for i, s in enumerate(seqs))


def recs_of(text, which):
    return b"".join(b"".join(rule.records(text)[0][r]) for r in which)


# ------------------------------------------------------------------------------------------------ the hand example
@pytest.mark.parametrize("nl", [b"\n", b"\r\n"])
def test_six_records_by_hand(nl):
    text = fq(SEQS, nl)
    got = rule.run(text, high=2)
    assert got["rows"].tolist() == [[5, 0], [5, 0], [5, 2], [3, 3], [0, 4], [0, 4]] and got["keep"].tolist() == [1, 0, 1, 1, 1, 0]
    assert got["out"] == recs_of(text, [0, 2, 3, 4]) and got["levels"].tolist() == [0, 2, 2, 0]
    assert got["figures"] == dict(records=6, records_out=4, distinct=4, duplicates=2, max_copies=2, bases_in=18, bases_out=13,
                                  bytes_out=len(got["out"]), lines=24)
    assert rule.run(text, high=1)["levels"].tolist() == [0, 2, 2]
    dup = rule.run(text, which=2)
    assert dup["out"] == recs_of(text, [1, 5]) and dup["keep"].tolist() == got["keep"].tolist() and dup["figures"]["records_out"] == 2
    # the first three bases: the proper prefix and the near miss fall in with the first read
    got = rule.run(text, prefix=3, high=2)
    assert got["rows"][:, 1].tolist() == [0, 0, 0, 0, 4, 4] and got["levels"].tolist() == [0, 0, 1, 1] and got["out"] == recs_of(text, [0, 4])
    assert rule.run(text, prefix=3, high=1)["levels"].tolist() == [0, 0, 2]
    assert rule.run(text, prefix=3, which=2)["out"] == recs_of(text, [1, 2, 3, 5])
    # pairs: (ACGTA, ACGTA), (ACGTC, ACG), ("", "") are three clusters; by three bases the first two are one
    got = rule.run(text, paired=1, high=2)
    assert got["rows"][:, 1].tolist() == [0, 1, 2, 3, 4, 5] and got["levels"].tolist() == [0, 3, 0, 0] and got["out"] == text
    assert rule.run(text, paired=1, which=2)["out"] == b""
    got = rule.run(text, paired=1, prefix=3, high=2)
    assert got["rows"][:, 1].tolist() == [0, 1, 0, 1, 4, 5] and got["keep"].tolist() == [1, 1, 0, 0, 1, 1]
    assert got["levels"].tolist() == [0, 1, 1, 0] and got["figures"]["distinct"] == 2 and got["figures"]["duplicates"] == 2
    assert rule.run(text, paired=1, prefix=3, which=2)["out"] == recs_of(text, [2, 3])
    assert rule.run(text, paired=1, prefix=3, high=1)["levels"].tolist() == [0, 1, 1]


def test_the_rule_takes_bytes_as_they_stand_and_names_errors():
    text = fq([b"acgt", b"ACGT", b"ACGN", b"ACGT"])
    assert rule.run(text)["rows"][:, 1].tolist() == [0, 1, 2, 1]
    assert rule.run(text[:-1])["out"] == recs_of(text, [0, 1, 2])  # (an open last line: nothing emitted is cut)
    assert rule.run(fq([b"AC", b"AC"])[:-1], which=2)["out"] == b"@r1\nAC\n+\nII\n"  # (the forced newline)
    assert rule.run(b"")["levels"].tolist() == [0] * 102 and rule.run(b"\n\n")["figures"]["records"] == 0
    for bad in (dict(which=0), dict(which=3), dict(high=0), dict(high=rule.MAX_HIGH + 1), dict(paired=2)):
        with pytest.raises(rule.DedupError) as e:
            rule.run(text, **bad)
        assert e.value.code == rule.ERR_ARG
    with pytest.raises(rule.DedupError) as e:
        rule.run(fq([b"A"] * 3), paired=1)
    assert e.value.code == rule.ERR_RANGE
    with pytest.raises(rule.DedupError) as e:
        rule.run(text, cap=3)
    assert e.value.code == rule.ERR_RANGE and e.value.counts == (4, 3)
    for spoiled, kind in ((text.replace(b"@r2", b">r2"), "at"), (text.replace(b"ACGN\n+", b"ACGN\n-"), "plus"),
                          (text.replace(b"ACGN", b"ACGNN"), "length")):
        with pytest.raises(rule.DedupError) as e:
            rule.run(spoiled)
        assert (e.value.code, e.value.record, e.value.kind) == (rule.ERR_UNSUPPORTED, 2, kind)
    with pytest.raises(rule.DedupError) as e:
        rule.run(text + b"@r4\nAC\n")
    assert (e.value.record, e.value.kind) == (4, "incomplete")


# ---------------------------------------------------------------------------------------------------- the writers
def test_writers_byte_for_byte():
    text = fq(SEQS)
    got = rule.run(text, high=2)
    names = kmers.fastq_names(text)
    copies = report.dedup_copies(got["rows"])
    assert copies == [2, 2, 1, 1, 2, 2]
    assert report.format_dedup_tsv(names, got["rows"], got["keep"], copies) == (
        b"record\tlength\tfirst\tcopies\tkeep\n"
        b"r0\t5\tr0\t2\t1\nr1\t5\tr0\t2\t0\nr2\t5\tr2\t1\t1\nr3\t3\tr3\t1\t1\nr4\t0\tr4\t2\t1\nr5\t0\tr4\t2\t0\n")
    assert report.format_dedup_levels(got["levels"], 6) == (b"copies\tsequences\treads\tpercent_of_reads\n"
                                                             b"1\t2\t2\t33.3333\n2\t2\t4\t66.6667\n>2\t0\t0\t0.0000\n")
    assert report.format_dedup_levels(rule.run(text, high=1)["levels"], 6) == (b"copies\tsequences\treads\tpercent_of_reads\n"
                                                                                b"1\t2\t2\t33.3333\n>1\t2\t4\t66.6667\n")
    assert report.format_dedup_levels(rule.run(b"")["levels"], 0) == b"copies\tsequences\treads\tpercent_of_reads\n>100\t0\t0\t0.0000\n"
    assert report.format_dedup_summary(got["figures"]) == (b"metric\tvalue\nreads\t6\ndistinct\t4\nduplicates\t2\nduplication_rate\t0.333333\n"
                                                           b"largest_cluster\t2\nbases_before\t18\nbases_after\t13\n")
    pairs = rule.run(text, paired=1, prefix=3)
    assert report.dedup_copies(pairs["rows"], paired=True) == [2, 2, 2, 2, 1, 1]
    assert report.format_dedup_summary(pairs["figures"], paired=True).split(b"\n")[1:5] == [b"pairs\t3", b"distinct\t2", b"duplicates\t1",
                                                                                           b"duplication_rate\t0.333333"]
    with pytest.raises(ValueError):
        report.format_dedup_tsv(names[:-1], got["rows"], got["keep"], copies)


def test_overrepresented_order_ties_and_limit():
    # clusters: r0 x2, r2 x1, r3 x1, r4 x2 -- the tie of two copies goes to the lower first; singletons never count
    text = fq(SEQS)
    got = rule.run(text)
    copies = report.dedup_copies(got["rows"])
    over = report.dedup_over(copies, got["rows"], over_frac=0.0)
    assert over == [(0, 2), (4, 2)]
    keys = kmers.fastq_keys(text)
    assert report.format_dedup_over(over, kmers.fastq_names(text), keys, 6) == (b"first\tcopies\tpercent\tsequence\n"
                                                                               b"r0\t2\t33.3333\tACGTA\nr4\t2\t33.3333\t\n")
    assert report.dedup_over(copies, got["rows"], over_frac=0.34) == [] and report.dedup_over(copies, got["rows"], over_frac=1 / 3) == over
    # more copies first, whatever the index; then the limit
    seqs = [b"AA", b"CC", b"CC", b"GG", b"CC", b"AA", b"TT", b"GG", b"GG", b"GG"]
    got = rule.run(fq(seqs))
    over = report.dedup_over(report.dedup_copies(got["rows"]), got["rows"], over_frac=0.2)
    assert over == [(3, 4), (1, 3), (0, 2)]
    assert report.dedup_over(report.dedup_copies(got["rows"]), got["rows"], over_frac=0.0, limit=2) == [(3, 4), (1, 3)]
    assert report.DEDUP_OVER_LIMIT == 1000
    # pairs: the first mate's record stands for the pair, both keys are written
    text = fq([b"AC", b"GT", b"AC", b"GT", b"AC", b"GG"])
    got = rule.run(text, paired=1)
    copies = report.dedup_copies(got["rows"], paired=True)
    over = report.dedup_over(copies, got["rows"], paired=True, over_frac=0.5)
    assert copies == [2, 2, 2, 2, 1, 1] and over == [(0, 2)]
    assert report.format_dedup_over(over, kmers.fastq_names(text), kmers.fastq_keys(text), 3, paired=True) == (
        b"first\tcopies\tpercent\tsequence\tsequence2\nr0\t2\t66.6667\tAC\tGT\n")
    assert kmers.fastq_keys(fq([b"ACGT", b"A"], b"\r\n"), prefix=2) == [b"AC", b"A"]


# ----------------------------------------------------------------------------------------- header and bindings
CTYPE = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double}


def _struct_fields(name):
    """[(C type, field)] of a struct of the header."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if stmt:
            ctype, rest = stmt.split(" ", 1)
            out += [(ctype, f.strip()) for f in rest.split(",")]
    return out


def test_header_declares_the_calls_and_the_version_stands():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ("mk_fastq_dedup_text", "mk_fastq_dedup_device"):
        assert name in native.ABI_SYMBOLS and getattr(native.lib(), name) is not None
    args = re.search(r"int mk_fastq_dedup_text\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["ctx", "fastq", "n", "piece_bytes", "opt", "cap", "keep", "rows", "levels",
                                                                   "out", "out_cap", "out_len", "nrec", "st"]
    args = re.search(r"int mk_fastq_dedup_device\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["ctx", "d_fastq", "n", "opt", "cap", "d_keep", "d_rows", "d_levels",
                                                                   "d_out", "out_cap", "out_len", "nrec", "st"]
    assert len(native.lib().mk_fastq_dedup_text.argtypes) == 14 and len(native.lib().mk_fastq_dedup_device.argtypes) == 13
    assert re.search(r"#define MK_DEDUP_MAX_HIGH \(1u << 20\)", code) and native.DEDUP_MAX_HIGH == 1 << 20 == rule.MAX_HIGH
    rule_text = " ".join(HEADER.split("duplicate reads of a FASTQ text")[1].split("#define MK_DEDUP_MAX_HIGH")[0].replace(" * ", " ").split())
    for phrase in ("a hash only chooses where to look", "'a' is not 'A'", "no reverse complement", "An empty read has the empty key",
                   "an odd record count is MK_ERR_RANGE", "lowest index over the whole call", "keep[r] = 1 iff first == r",
                   "levels[high + 1] = those of more", "keep, rows and levels may each be NULL", "aligned to 8", "MK_ERR_NOMEM",
                   "Nothing depends on piece_bytes", "The text is never written"):
        assert phrase in rule_text, phrase
    assert native.MK_ABI == 6 and native.lib().mk_version().decode() == "mercat_hip 6.1 (gfx950)"


def test_bound_structs_match_the_header():
    fields = _struct_fields("mk_dedup_opt_t")
    assert [(CTYPE[t], f) for t, f in fields] == [(t, f) for f, t in native.DedupOpt._fields_] and C.sizeof(native.DedupOpt) == 16
    assert [f for _, f in fields] == ["prefix", "paired", "which", "high"]
    fields = _struct_fields("mk_fastq_dedup_t")
    assert [f for _, f in fields] == ["records", "records_out", "distinct", "duplicates", "max_copies", "slots", "probes", "compares",
                                      "bases_in", "bases_out", "bytes_out", "lines", "s_plan", "s_copy", "s_index", "s_scan", "s_key",
                                      "s_insert", "s_place", "s_gather", "s_levels", "s_write"]
    assert [(CTYPE[t], f) for t, f in fields] == [(t, f) for f, t in native.FastqDedup._fields_]
    assert [getattr(native.FastqDedup, f).offset for _, f in fields] == list(range(0, 176, 8)) and C.sizeof(native.FastqDedup) == 176
    st = native.FastqDedup()
    st.distinct, st.s_insert = 3, 0.5
    assert st.as_dict()["distinct"] == 3 and st.as_dict()["s_insert"] == 0.5 and set(st.as_dict()) == {f for _, f in fields}


def test_python_layers_are_there():
    assert list(inspect.signature(native.Counter.fastq_dedup).parameters)[1:] == ["path_or_bytes", "prefix", "paired", "which", "high",
                                                                                 "piece_bytes", "info"]
    d = {k: p.default for k, p in inspect.signature(native.Counter.fastq_dedup).parameters.items()}
    assert (d["prefix"], d["paired"], d["which"], d["high"], d["piece_bytes"], d["info"]) == (0, False, 1, 100, 0, None)
    assert callable(native.Counter.fastq_dedup_device) and native.DEDUP_COLUMNS == ("length", "first")
    opt = native.dedup_options(prefix=50, paired=True, which=2, high=7)
    assert (opt.prefix, opt.paired, opt.which, opt.high) == (50, 1, 2, 7)
    for bad in (dict(prefix=-1), dict(high=1 << 32)):
        with pytest.raises(ValueError):
            native.dedup_options(**bad)
    names = list(inspect.signature(kmers.dedup_reads).parameters)
    assert names == ["file", "out_path", "prefix", "paired", "keep", "high", "over_frac", "tsv_path", "summary_path", "levels_path",
                     "over_path", "mate_file", "out_path2", "device", "keep_text"]
    d = {k: p.default for k, p in inspect.signature(kmers.dedup_reads).parameters.items()}
    assert (d["prefix"], d["paired"], d["keep"], d["high"], d["over_frac"], d["device"], d["keep_text"]) == (0, False, "unique", 100, 0.001, 0,
                                                                                                           False)
    with pytest.raises(ValueError):  # (before any call of the library)
        kmers.dedup_reads("reads.fna", None)
    with pytest.raises(ValueError):
        kmers.dedup_reads(b"", None, keep="best")


# ------------------------------------------------------------------------------------------------ the command line
@pytest.fixture()
def files(tmp_path):
    (tmp_path / "s.fna").write_bytes(b">a\nACGTACGTAC\n")
    (tmp_path / "r.fastq").write_bytes(b"@a\nACGTACGTAC\n+\nIIIIIIIIII\n")
    return tmp_path


def parse(files, inputs, *extra):
    return cli.parseargs(list(inputs) + ["-k", "5", "-o", str(files / "out")] + [str(x) for x in extra])[0]


def test_cli_accepts_dedup(files):
    args = parse(files, ["-i", str(files / "r.fastq")], "-dedup")
    assert args.dedup is True and args.dedup_prefix is None and args.dedup_paired is False and not args.skipclean
    assert cli.classify(files / "r.fastq", args.skipclean or args.dedup)[0] == "nucleotide"  # (with or without -skipclean)
    args = parse(files, ["-i", str(files / "r.fastq")], "-dedup", "-dedup_prefix", 50, "-dedup_paired", "-dedup_high", 10, "-dedup_over", 0.01,
                 "-skipclean")
    assert (args.dedup_prefix, args.dedup_paired, args.dedup_high, args.dedup_over) == (50, True, 10, 0.01)
    assert parse(files, ["-i", str(files / "r.fastq")], "-skipclean").dedup is False
    doc = " ".join(cli.__doc__.split())
    assert "-dedup takes FASTQ input" in doc and "mk_fastq_dedup_text" in doc and "before -overlap, -adapt and -qtrim" in doc


@pytest.mark.parametrize("extra,message", [
    (["-dedup_prefix", 10], "-dedup_prefix needs -dedup"),
    (["-dedup_paired"], "-dedup_paired needs -dedup"),
    (["-dedup_high", 10], "-dedup_high needs -dedup"),
    (["-dedup_over", 0.5], "-dedup_over needs -dedup"),
    (["-dedup", "-dedup_high", 0], "-dedup_high 0: must lie in 1..1048576"),
    (["-dedup", "-dedup_high", (1 << 20) + 1], "must lie in 1..1048576"),
    (["-dedup", "-dedup_prefix", -1], "-dedup_prefix -1: must lie in"),
    (["-dedup", "-dedup_over", 1.5], "-dedup_over 1.5: must lie in 0..1"),
])
def test_cli_refuses(files, capsys, extra, message):
    with pytest.raises(SystemExit) as e:
        parse(files, ["-i", str(files / "r.fastq")], "-skipclean", *extra)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_cli_refuses_dedup_without_fastq_input(files, capsys):
    with pytest.raises(SystemExit) as e:
        parse(files, ["-i", str(files / "s.fna")], "-dedup")
    assert e.value.code == 2 and "no input is a FASTQ file" in capsys.readouterr().err
