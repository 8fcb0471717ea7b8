"""The overlap rule (tests/overlap_rule.py) against pairs worked by hand and against itself on fragments it must recover,
and the parts of mk_fastq_overlap_*'s Python layers that need no GPU: the header and the bindings, the option checks, the
reports and the command line."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import overlap_rule as rule
from conftest import ROOT
from mercat2_amd import cli, kmers, native, report

HEADER = (ROOT / "include" / "mercat_hip.h").read_text()
NO = rule.NO_HIT
STRICT = dict(max_mismatch=0, max_err_ppm=0)


def fq(*seqs, quals=None, nl=b"\n"):
    quals = quals or [b"I" * len(s) for s in seqs]
    return b"".join(b"@r%d" % i + nl + s + nl + b"+" + nl + q + nl for i, (s, q) in enumerate(zip(seqs, quals)))


# ---------------------------------------------------------------------------------------------------- the rule
def test_the_notation():
    assert rule.revcomp(b"ACGTacgtNx.") == b"NNNACGTACGT"
    assert rule.revcomp(b"NTTCGT") == b"ACGAAN"
    assert list(rule.candidates(10, 9, 4)) == [0, 1, 2, 3, 4, 5, 6, -1, -2, -3, -4, -5]
    assert list(rule.candidates(14, 6, 6)) == [0, 1, 2, 3, 4, 5, 6, 7, 8] and list(rule.candidates(6, 14, 6)) == [0, -1, -2, -3, -4, -5, -6, -7, -8]
    assert list(rule.candidates(5, 9, 6)) == [] and list(rule.candidates(6, 6, 6)) == [0]


def test_hand_pairs_offset_zero_positive_negative_and_contained():
    # d = 0: the mates cover the same 8 bases
    assert rule.find(b"ACGTTGCA", b"TGCAACGT", 4, 0, 0) == (0, 8, 8, 0)
    # d = 5: GGGGGACGTA over .....ACGTACCCC; offsets 0 .. 4 put a G of mate 1 over the leading A of rc
    assert rule.find(b"GGGGGACGTA", b"GGGGTACGT", 4, 0, 0) == (5, 14, 5, 0)
    # d = -2, read-through: the fragment CATTGACA, GG and (on mate 2's strand) AA behind it
    assert rule.find(b"CATTGACAGG", b"TGTCAATGAA", 6, 0, 0) == (-2, 8, 8, 0)
    # mate 2 shorter and contained: TTTTACGTCATTTT over ....ACGTCA
    assert rule.find(b"TTTTACGTCATTTT", b"TGACGT", 6, 0, 0) == (4, 10, 6, 0)
    text = fq(b"ACGTTGCA", b"TGCAACGT", b"GGGGGACGTA", b"GGGGTACGT", b"CATTGACAGG", b"TGTCAATGAA", b"TTTTACGTCATTTT", b"TGACGT",
              quals=[b"ABCDEFGH", b"abcdefgh", b"ABCDEFGHIJ", b"abcdefghi", b"ABCDEFGHIJ", b"abcdefghij", b"ABCDEFGHIJKLMN", b"abcdef"])
    trim = rule.run(text, mode=rule.TRIM, min_overlap=4, **STRICT)
    assert trim["rows"] == [(8, 8, 8, 8, 0), (8, 8, 8, 8, 0), (10, 10, 14, 5, 0), (9, 9, 14, 5, 0), (10, 8, 8, 8, 0), (10, 8, 8, 8, 0),
                            (14, 10, 10, 6, 0), (6, 6, 10, 6, 0)]
    assert trim["keep"] == [1] * 8
    assert trim["out"] == (b"@r0\nACGTTGCA\n+\nABCDEFGH\n@r1\nTGCAACGT\n+\nabcdefgh\n@r2\nGGGGGACGTA\n+\nABCDEFGHIJ\n@r3\nGGGGTACGT\n+\nabcdefghi\n"
                           b"@r4\nCATTGACA\n+\nABCDEFGH\n@r5\nTGTCAATG\n+\nabcdefgh\n@r6\nTTTTACGTCA\n+\nABCDEFGHIJ\n@r7\nTGACGT\n+\nabcdef\n")
    f = trim["figures"]
    assert (f["pairs"], f["pairs_hit"], f["pairs_trimmed"], f["pairs_merged"], f["records_out"], f["records_trimmed"]) == (4, 4, 2, 0, 8, 3)
    assert (f["bases_in"], f["bases_out"], f["bytes_out"]) == (75, 67, len(trim["out"]))
    merge = rule.run(text, mode=rule.MERGE, min_overlap=4, **STRICT)
    assert merge["rows"] == trim["rows"] and merge["keep"] == [1] * 8
    # lower case letters of the ASCII table are above the upper case ones: mate 2's quality bytes win every overlap position
    assert merge["out"] == (b"@r0\nACGTTGCA\n+\nhgfedcba\n@r2\nGGGGGACGTACCCC\n+\nABCDEihgfedcba\n@r4\nCATTGACA\n+\nhgfedcba\n"
                            b"@r6\nTTTTACGTCA\n+\nABCDfedcba\n")
    f = merge["figures"]
    assert (f["pairs_merged"], f["pairs_trimmed"], f["records_out"], f["records_trimmed"], f["bases_out"]) == (4, 0, 4, 4, 40)
    assert rule.run(text, mode=rule.MERGE, which=2, min_overlap=4, **STRICT)["out"] == b""
    # a fragment below min_len drops the pair in both modes; without a hit a pair is whole (trim) or unmerged (merge)
    short = rule.run(text, mode=rule.MERGE, min_overlap=4, min_len=9, **STRICT)
    assert short["keep"] == [0, 0, 1, 1, 0, 0, 1, 1] and short["figures"]["dropped_short"] == 2
    assert rule.run(text, mode=rule.TRIM, min_overlap=4, min_len=9, **STRICT)["keep"] == [0, 0, 1, 1, 0, 0, 1, 1]
    none = rule.run(text, mode=rule.MERGE, which=2, min_overlap=9, **STRICT)
    assert none["keep"] == [2] * 8 and none["out"] == text and none["rows"][0] == (8, 8, NO, 0, 0)
    assert rule.run(text, mode=rule.TRIM, min_overlap=9, **STRICT)["out"] == text


def test_hand_consensus_ties_n_and_lower_case():
    # s1 AcNTAC over rc ACGAAN, position by position: equal; equal (folded), mate 1's letter stays; N against G: the base
    # wins with its own quality; T against A: the higher quality wins; equal; C against N: the base wins, whatever N's quality
    assert rule.merged(b"AcNTAC", b"5I5555", b"NTTCGT", b"~5I!5I", 0) == (b"AcGAAC", b"II!I55")
    assert rule.merged(b"T", b"5", b"T", b"5", 0) == (b"T", b"5")  # a tie: mate 1
    assert rule.merged(b"T", b"5", b"T", b"6", 0) == (b"A", b"6")
    assert rule.merged(b"N", b"9", b"n", b"9", 0) == (b"N", b"9") and rule.merged(b"n", b"8", b".", b"9", 0) == (b"N", b"9")
    # N in either mate is a mismatch, lower case is none
    assert rule.find(b"acgttgca", b"TGCAACGT", 4, 0, 0) == (0, 8, 8, 0)
    assert rule.find(b"ACGTTGCA", b"TGCAACNT", 8, 0, 1000000) is None and rule.find(b"ACGTTGCA", b"TGCAACNT", 8, 1, 1000000) == (0, 8, 8, 1)
    assert rule.find(b"ANGTTGCA", b"TGCAACNT", 8, 1, 1000000) == (0, 8, 8, 1)  # N against N: one position, one mismatch
    assert rule.find(b"ANGTTGCA", b"TGNAACGT", 8, 1, 1000000) is None and rule.find(b"ANGTTGCA", b"TGNAACGT", 8, 2, 1000000) == (0, 8, 8, 2)


def test_hand_limits_overlap_count_and_rate():
    O = b"ACGTTGCAAC"
    s1 = b"GGGGG" + O

    def s2_with(k):  # rc = O with its first k bases substituted, then CCCCC
        return rule.revcomp(O[:k].translate(bytes.maketrans(b"ACGT", b"CATG")) + O[k:] + b"CCCCC")
    assert rule.find(s1, s2_with(0), 10, 5, 200000) == (5, 20, 10, 0)
    assert rule.find(s1, s2_with(0), 11, 5, 200000) is None  # ov exactly min_overlap, and one more asked
    assert rule.find(s1, s2_with(2), 10, 5, 200000) == (5, 20, 10, 2)  # 2 * 10^6 <= 200000 * 10
    assert rule.find(s1, s2_with(2), 10, 5, 199999) is None
    assert rule.find(s1, s2_with(3), 10, 5, 200000) is None and rule.find(s1, s2_with(3), 10, 5, 300000) == (5, 20, 10, 3)
    assert rule.find(s1, s2_with(2), 10, 2, 1000000) == (5, 20, 10, 2) and rule.find(s1, s2_with(2), 10, 1, 1000000) is None
    # six allowed at any rate: offset 4 comes first in the order, and GACGTTGCAAC over CATGGTCAACC differs at six of 11 too
    assert rule.find(s1, s2_with(6), 10, 5, 1000000) is None and rule.find(s1, s2_with(6), 10, 6, 1000000) == (4, 19, 11, 6)
    assert rule.find(s1, s2_with(6), 10, 6, 545454) is None and rule.find(s1, s2_with(6), 10, 6, 545455) == (4, 19, 11, 6)
    # a mate above 512 bases: not tested, counted
    long_ = rule.run(fq(b"A" * 513, b"T" * 513, b"A" * 512, b"T" * 512), min_overlap=30)
    assert long_["rows"] == [(513, 513, NO, 0, 0)] * 2 + [(512, 512, 512, 512, 0)] * 2 and long_["figures"]["skipped_long"] == 1


def test_the_rule_recovers_planted_fragments():
    rng = np.random.default_rng(1)
    L = 60
    seq = lambda n: bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))
    for F in range(30, 2 * L - 30 + 1):
        frag, a1, a2 = seq(F), seq(L), seq(L)
        s1, s2 = (frag + a1)[:L], (rule.revcomp(frag) + a2)[:L]
        assert rule.find(s1, s2, 30, 5, 200000) == (F - L, F, min(F, L) - max(F - L, 0), 0)
        got = rule.run(fq(s1, s2), mode=rule.MERGE)
        assert got["out"] == b"@r0\n" + frag + b"\n+\n" + b"I" * F + b"\n" and got["rows"][0][1:] == (min(L, F), F, min(F, 2 * L - F), 0)
        cut = rule.run(fq(s1, s2), mode=rule.TRIM)
        assert cut["out"] == fq(frag[:L], rule.revcomp(frag)[:L])


def test_the_rule_refuses_what_the_call_refuses():
    text = fq(b"ACGTTGCA", b"TGCAACGT")
    for kw in (dict(mode=2), dict(min_overlap=0), dict(min_overlap=513), dict(max_err_ppm=1000001), dict(which=0), dict(which=3),
               dict(mode=rule.TRIM, which=2)):
        with pytest.raises(rule.OverlapError) as e:
            rule.run(text, **kw)
        assert e.value.code == rule.ERR_ARG
    with pytest.raises(rule.OverlapError) as e:
        rule.run(text + fq(b"ACGT"), min_overlap=4)
    assert e.value.code == rule.ERR_RANGE and e.value.counts == (3,)
    with pytest.raises(rule.OverlapError) as e:
        rule.run(text, cap=1)
    assert e.value.code == rule.ERR_RANGE and e.value.counts == (2, 1)
    with pytest.raises(rule.OverlapError) as e:
        rule.run(text + b"@x\nACGT\n-\nIIII\n@y\nACGT\n+\nIIII\n")
    assert (e.value.code, e.value.record, e.value.kind) == (rule.ERR_UNSUPPORTED, 2, "plus")
    # CR LF, an open end and trailing empty lines are tolerated; uncut records keep their bytes
    crlf = fq(b"ACGTTGCA", b"TGCAACGT", nl=b"\r\n")
    assert rule.run(crlf, mode=rule.TRIM, min_overlap=4)["out"] == crlf
    assert rule.run(crlf[:-2] + b"\n\n", mode=rule.MERGE, which=2, min_overlap=9)["out"] == crlf[:-2] + b"\n"
    assert rule.run(crlf, mode=rule.MERGE, min_overlap=4)["out"] == b"@r0\r\nACGTTGCA\n+\r\nIIIIIIII\n"


# ----------------------------------------------------------------------------------------- header and bindings
CTYPE = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double}


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
    for name in ("mk_fastq_overlap_text", "mk_fastq_overlap_device"):
        assert name in native.ABI_SYMBOLS and getattr(native.lib(), name) is not None
    args = re.search(r"int mk_fastq_overlap_text\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "ctx", "fastq", "n", "piece_bytes", "opt", "cap", "keep", "rows", "out", "out_cap", "out_len", "nrec", "st"]
    args = re.search(r"int mk_fastq_overlap_device\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "ctx", "d_fastq", "n", "opt", "cap", "d_keep", "d_rows", "d_out", "out_cap", "out_len", "nrec", "st"]
    assert len(native.lib().mk_fastq_overlap_text.argtypes) == 13 and len(native.lib().mk_fastq_overlap_device.argtypes) == 12
    assert re.search(r"#define MK_OVERLAP_MAX_BASES (\d+)", code).group(1) == str(native.OVERLAP_MAX_BASES) == str(rule.MAX_BASES)
    assert native.lib().mk_version().decode().split()[1] == "6.1"


def test_bound_structs_match_the_header():
    fields = _struct_fields("mk_overlap_opt_t")
    assert [f for _, f in fields] == ["mode", "min_overlap", "max_mismatch", "max_err_ppm", "min_len", "which"] == list(rule.OPT)
    assert [(CTYPE[t], f) for t, f in fields] == [(t, f) for f, t in native.OverlapOpt._fields_] and C.sizeof(native.OverlapOpt) == 24
    fields = _struct_fields("mk_fastq_overlap_t")
    assert [f for _, f in fields] == ["records", "pairs", "pairs_hit", "pairs_merged", "pairs_trimmed", "dropped_short", "skipped_long",
                                      "records_out", "records_trimmed", "bases_in", "bases_out", "bytes_out", "lines", "s_copy", "s_index",
                                      "s_scan", "s_place", "s_gather", "s_write"]
    assert [(CTYPE[t], f) for t, f in fields] == [(t, f) for f, t in native.FastqOverlap._fields_]
    assert [getattr(native.FastqOverlap, f).offset for _, f in fields] == [8 * i for i in range(19)] and C.sizeof(native.FastqOverlap) == 152


def test_python_layers_are_there():
    assert list(inspect.signature(native.Counter.fastq_overlap).parameters)[1:] == [
        "path_or_bytes", "mode", "min_overlap", "max_mismatch", "max_err", "min_len", "which", "piece_bytes", "info"]
    d = {k: p.default for k, p in inspect.signature(native.Counter.fastq_overlap).parameters.items()}
    assert (d["mode"], d["min_overlap"], d["max_mismatch"], d["max_err"], d["min_len"], d["which"]) == ("merge", 30, 5, 0.2, 0, 1)
    assert callable(native.Counter.fastq_overlap_device) and native.OVERLAP_COLUMNS == ("length", "kept", "fragment", "overlap", "mismatches")
    opt = native.overlap_options()
    assert tuple(getattr(opt, f) for f, _ in native.OverlapOpt._fields_) == tuple(rule.OPT.values())
    opt = native.overlap_options("trim", 12, 3, 0.25, 40, 1)
    assert (opt.mode, opt.min_overlap, opt.max_mismatch, opt.max_err_ppm, opt.min_len, opt.which) == (0, 12, 3, 250000, 40, 1)
    assert native.overlap_options(1).mode == 1 and native.overlap_options(0).mode == 0
    for bad in (dict(mode="join"), dict(mode=True), dict(max_err=1.5), dict(min_len=-1), dict(min_overlap=1 << 32), dict(max_mismatch=-1)):
        with pytest.raises(ValueError):
            native.overlap_options(**bad)
    names = list(inspect.signature(kmers.overlap_reads).parameters)
    assert names[:3] == ["file", "out_path", "mode"] and inspect.signature(kmers.overlap_reads).parameters["mode"].default == "merge"
    assert {"min_overlap", "max_mismatch", "max_err", "min_len", "mate_file", "out_path2", "unmerged_path", "unmerged_path2", "tsv_path",
            "summary_path", "device"} <= set(names)
    for args, kw in ((("reads.fna", "out.fastq"), {}), (("reads.fastq", "out.fastq"), dict(mode="join")),
                     (("reads.fastq", "out.fastq"), dict(out_path2="o2.fastq")), (("reads.fastq", "out.fastq"), dict(mode="trim", unmerged_path="u.fastq")),
                     (("reads.fastq", "out.fastq"), dict(unmerged_path2="u2.fastq")), (("reads.fastq", "out.fastq"), dict(max_err=2.0)),
                     (("reads.fastq", "out.fastq"), dict(mate_file="mates.fna"))):
        with pytest.raises(ValueError):  # (before a file is read or the library called)
            kmers.overlap_reads(*args, **kw)


def test_the_reports():
    text = fq(b"GGGGGACGTA", b"GGGGTACGT", b"CATTGACAGG", b"TGTCAATGAA", b"AAAAAAAA", b"CCCCCCCC", b"ACGTTGCA", b"TGCAACGT")
    got = rule.run(text, mode=rule.TRIM, min_overlap=4, min_len=9, **STRICT)
    names = ["r%d" % i for i in range(8)]
    assert report.format_overlap_tsv(names, got["rows"], got["keep"]) == (
        b"record\tlength\tkept\tfragment\toverlap\tmismatches\tkeep\nr0\t10\t10\t14\t5\t0\t1\nr1\t9\t9\t14\t5\t0\t1\n"
        b"r2\t10\t8\t8\t8\t0\t0\nr3\t10\t8\t8\t8\t0\t0\nr4\t8\t8\t-\t0\t0\t1\nr5\t8\t8\t-\t0\t0\t1\nr6\t8\t8\t8\t8\t0\t0\nr7\t8\t8\t8\t8\t0\t0\n")
    fragments = report.overlap_fragments(np.array(got["rows"], np.uint64))
    assert fragments == {8: 2, 14: 1} and list(fragments) == [8, 14]
    assert report.format_overlap_summary(got["figures"], fragments) == (
        b"metric\tbefore\tafter\nreads\t8\t4\nbases\t71\t35\npairs\t\t4\nhits\t\t3\nmerged\t\t0\ntrimmed\t\t0\ndropped_short\t\t2\n"
        b"skipped_long\t\t0\nfragment\tpairs\n8\t2\n14\t1\n")
    with pytest.raises(ValueError):
        report.format_overlap_tsv(["r0"], got["rows"], got["keep"])


# ------------------------------------------------------------------------------------------------ the command line
@pytest.fixture()
def files(tmp_path):
    (tmp_path / "s.fna").write_bytes(b">a\nACGTACGTAC\n")
    (tmp_path / "r.fastq").write_bytes(b"@a\nACGTACGTAC\n+\nIIIIIIIIII\n")
    (tmp_path / "r2.fastq").write_bytes(b"@a\nACGTACGTAC\n+\nIIIIIIIIII\n")
    return tmp_path


def parse(files, inputs, *extra):
    return cli.parseargs(list(inputs) + ["-k", "5", "-o", str(files / "out")] + [str(x) for x in extra])[0]


def test_cli_accepts_overlap(files):
    args = parse(files, ["-i", str(files / "r.fastq")], "-overlap", "merge")
    assert (args.overlap, args.overlap_min, args.overlap_diff, args.overlap_err, args.overlap_len, args.overlap_mate) == ("merge", None, None, None, None, None)
    args = parse(files, ["-i", str(files / "s.fna"), str(files / "r.fastq")], "-overlap", "trim", "-overlap_min", 12, "-overlap_diff", 3,
                 "-overlap_err", 0.1, "-overlap_len", 40, "-overlap_mate", files / "r2.fastq", "-adapt", "-qtrim", "-skipclean")
    assert (args.overlap, args.overlap_min, args.overlap_diff, args.overlap_err, args.overlap_len) == ("trim", 12, 3, 0.1, 40)
    assert args.overlap_mate == str(files / "r2.fastq") and args.adapt == "" and args.qtrim == 20
    assert parse(files, ["-i", str(files / "r.fastq")]).overlap is None


def test_the_help_says_what_stays_out(capsys):
    with pytest.raises(SystemExit) as e:
        cli.parseargs(["-h"])
    help_ = " ".join(capsys.readouterr().out.split())
    assert e.value.code == 0 and "-overlap {trim,merge}" in help_ and "-overlap_mate FILE2" in help_
    assert "no mate-overlap detection" not in help_ and "poly-G trimming stay out" in help_ and "fastp -c" in help_
    assert "mate-overlap detection and poly-G trimming stay out" not in " ".join(cli.__doc__.split()) and "fastp -c" in cli.__doc__


@pytest.mark.parametrize("extra,message", [
    (["-overlap_min", 10], "-overlap_min needs -overlap"),
    (["-overlap_diff", 2], "-overlap_diff needs -overlap"),
    (["-overlap_err", 0.2], "-overlap_err needs -overlap"),
    (["-overlap_len", 10], "-overlap_len needs -overlap"),
    (["-adapt", "-overlap_mate", "r2.fastq"], "-overlap_mate needs -overlap"),
    (["-overlap", "join"], "invalid choice"),
    (["-overlap", "merge", "-overlap_min", 0], "-overlap_min 0: must lie in 1..512"),
    (["-overlap", "merge", "-overlap_min", 513], "-overlap_min 513: must lie in 1..512"),
    (["-overlap", "trim", "-overlap_err", 1.5], "-overlap_err 1.5: must lie in 0..1"),
    (["-overlap", "trim", "-overlap_diff", -1], "-overlap_diff -1"),
    (["-overlap", "trim", "-overlap_len", -1], "-overlap_len -1"),
    (["-overlap", "merge", "-overlap_mate", "nowhere.fastq"], "file 'nowhere.fastq' is not valid"),
])
def test_cli_refuses(files, capsys, extra, message):
    with pytest.raises(SystemExit) as e:
        parse(files, ["-i", str(files / "r.fastq")], *extra)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_cli_refuses_a_mate_file_for_several_inputs_and_overlap_without_fastq_input(files, capsys):
    with pytest.raises(SystemExit) as e:
        parse(files, ["-i", str(files / "r.fastq"), str(files / "r2.fastq")], "-overlap", "merge", "-overlap_mate", files / "r2.fastq")
    assert e.value.code == 2 and "exactly one FASTQ input" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        parse(files, ["-i", str(files / "r.fastq")], "-overlap", "merge", "-overlap_mate", files / "s.fna")
    assert e.value.code == 2 and "needs a FASTQ file" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        parse(files, ["-i", str(files / "s.fna")], "-overlap", "trim")
    assert e.value.code == 2 and "no input is a FASTQ file" in capsys.readouterr().err
