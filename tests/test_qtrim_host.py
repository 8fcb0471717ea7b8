"""mk_fastq_qtrim_* without a GPU: the rule of tests/qtrim_rule.py on hand examples whose answers are written out, the
8-line cut scanner, the header, the bindings and the command line's refusals."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import qtrim_rule as rule
from conftest import ROOT
from mercat2_amd import cli, kmers, native, report

HEADER = (ROOT / "include" / "mercat_hip.h").read_text()


# --------------------------------------------------------------------------------------------------- the cut
@pytest.mark.parametrize("q,cut_front,cut_back,want", [
    # ties cut less: the sums 1, 0, 1 reach their maximum twice, the first counts (5': index 0; 3': index 4)
    ([19, 21, 19, 30, 30], 20, 0, (1, 5)),
    ([30, 30, 19, 21, 19], 0, 20, (0, 4)),
    # a sum that returns to exactly 0 does not stop the scan: 1, 0, 2
    ([19, 21, 18, 30, 30], 20, 0, (3, 5)),
    ([30, 30, 18, 21, 19], 0, 20, (0, 2)),
    # a larger maximum behind the first negative sum does not count: 1, -1 | 9
    ([19, 22, 10, 30, 30], 20, 0, (1, 5)),
    ([30, 30, 10, 22, 19], 0, 20, (0, 4)),
    # the first base is good: the sum is negative at once, nothing is cut although worse bases follow
    ([21, 2, 2, 2], 20, 0, (0, 4)),
    ([2, 2, 2, 21], 0, 20, (0, 4)),
    # both ends, each on the untrimmed read
    ([2, 30, 30, 30, 2, 2], 20, 20, (1, 4)),
    # start >= stop: all of it is poor; the 5' sweep takes all five, the 3' sweep too
    ([2, 2, 2, 2, 2], 20, 20, (0, 0)),
    ([2, 2, 2, 2, 2], 20, 0, (0, 0)),
    ([2, 2, 2, 2, 2], 0, 20, (0, 0)),
    # a cutoff of 0 never trims, whatever the qualities
    ([0, 0, 0, 0], 0, 0, (0, 4)),
    ([0, 40, 0], 0, 0, (0, 3)),
    # quality equal to the cutoff adds 0: no new maximum, no stop
    ([20, 20, 20], 20, 20, (0, 3)),
    # L of 0 and 1
    ([], 20, 20, (0, 0)),
    ([19], 20, 20, (0, 0)),
    ([19], 20, 0, (0, 0)),
    ([20], 20, 20, (0, 1)),
    ([30], 20, 20, (0, 1)),
])
def test_hand_examples_of_the_cut(q, cut_front, cut_back, want):
    assert rule.cut(q, cut_front, cut_back) == want


def fq(*reads):
    return b"".join(b"@r%d\n" % i + seq + b"\n+\n" + bytes(v + 33 for v in q) + b"\n" for i, (seq, q) in enumerate(reads))


def test_the_four_drop_reasons_in_their_order():
    reads = [(b"ACGTACGT", [30] * 8),                      # passes
             (b"ACGTACGT", [30, 30, 30, 2, 2, 2, 2, 2]),    # cut to 3: short
             (b"NNGTACGT", [30] * 8),                       # 2 N: n
             (b"ACGTACGT", [30, 30, 30, 30, 30, 12, 12, 30]),  # 2 of 8 below 15, more than 0.2: lowq
             (b"ACGTACGT", [26] * 8),                       # mean 26 < 28: meanq
             (b"NNGT", [12] * 4),                           # everything applies: the first names it
             (b"NNGTACGT", [12] * 8),                       # n before lowq before meanq
             (b"ACGTACGT", [12, 12] + [26] * 6)]            # lowq before meanq
    got = rule.run(fq(*reads), cut_back=10, min_len=5, max_n=1, low_q=15, max_low_ppm=200000, min_mean_q=28)
    assert got["reasons"] == [None, "short", "n", "lowq", "meanq", "short", "n", "lowq"]
    assert got["rows"][1] == (8, 0, 3, 0, 0, 90) and got["rows"][3] == (8, 0, 8, 0, 2, 204) and got["rows"][2][3] == 2
    assert got["keep"] == [1, 0, 0, 0, 0, 0, 0, 0] and got["out"] == fq(reads[0])
    f = got["figures"]
    assert (f["dropped_short"], f["dropped_n"], f["dropped_lowq"], f["dropped_meanq"], f["records_out"]) == (2, 2, 2, 1, 1)
    # exactly at the limits nothing is dropped: 1 N, 1 of 5 low, mean exactly 28
    edge = rule.run(fq((b"NCGTA", [28, 28, 28, 14, 42])), cut_back=0, min_len=5, max_n=1, low_q=15, max_low_ppm=200000, min_mean_q=28)
    assert edge["reasons"] == [None] and edge["rows"] == [(5, 0, 5, 1, 1, 140)]
    # min_len 0 still drops an emptied read, and hist counts the text and the emitted spans apart
    none = rule.run(fq((b"ACGT", [2] * 4), (b"AC", [30, 3])), cut_back=20, min_len=0)
    assert none["reasons"] == ["short", None] and none["out"] == b"@r1\nA\n+\n?\n"
    assert none["hist"][2] == 4 and none["hist"][30] == 1 and none["hist"][3] == 1 and sum(none["hist"][:256]) == 6
    assert none["hist"][256 + 30] == 1 and sum(none["hist"][256:]) == 1


def test_untrimmed_records_come_back_byte_for_byte():
    text = b"@a x\r\nACGT\r\n+a\r\nIIII\r\n@b\nAC\n+\nII"
    got = rule.run(text, cut_back=20)
    assert got["out"] == text + b"\n" and got["figures"]["records_trimmed"] == 0
    cut = rule.run(b"@a x\r\nACGT\r\n+a\r\nII##\r\n", cut_back=20)
    assert cut["out"] == b"@a x\r\nAC\n+a\r\nII\n" and cut["figures"]["records_trimmed"] == 1 and cut["rows"] == [(4, 0, 2, 0, 0, 80)]


def test_the_pair_rule():
    assert rule.pair_keep([True, True, True, False, False, True, False, False], True) == [1, 1, 2, 0, 0, 2, 0, 0]
    assert rule.pair_keep([True, False, True], False) == [1, 0, 1]
    good, poor = (b"ACGTAC", [30] * 6), (b"ACGTAC", [2] * 6)
    text = fq(good, good, good, poor, poor, good, poor, poor)
    main, orphans = rule.run(text, paired=1, which=1), rule.run(text, paired=1, which=2)
    recs = [b"".join(r) for r in rule.records(text)[0]]
    assert main["keep"] == orphans["keep"] == [1, 1, 2, 0, 0, 2, 0, 0]
    assert main["out"] == recs[0] + recs[1] and orphans["out"] == recs[2] + recs[5] and main["figures"]["orphans"] == 2
    assert sum(main["hist"][256:]) == 12 and sum(orphans["hist"][256:]) == 12 and main["hist"][:256] == orphans["hist"][:256]
    for bad in (dict(which=2), dict(which=0), dict(which=3, paired=1), dict(phred_base=34), dict(cut_back=94), dict(cut_front=94)):
        with pytest.raises(rule.QtrimError) as e:
            rule.run(text, **bad)
        assert e.value.code == rule.ERR_ARG
    with pytest.raises(rule.QtrimError) as e:
        rule.run(fq(good, good, good), paired=1)
    assert e.value.code == rule.ERR_RANGE
    with pytest.raises(rule.QtrimError) as e:
        rule.run(fq(good, good, good), cap=2)
    assert e.value.code == rule.ERR_RANGE and e.value.counts == (3, 2)


def test_the_checks_and_their_order():
    good = fq((b"ACGT", [30] * 4))
    for text, record, kind in ((b">r\nAC\n+\nII\n", 0, "at"), (good + b"@r\nAC\n-\nII\n", 1, "plus"), (good + b"@r\nAC\n+\nIII\n", 1, "length"),
                               (good + b"@r\nAC\n+\nI \n", 1, "qual"), (b">r\nAC\n-\nI \n", 0, "at"), (b"@r\nAC\n+\nI\n@s\nA\n+\n \n", 0, "length"),
                               (good + b"@r\nAC\n", 1, "incomplete"), (good + b"@r\nAC\n+\nI \n@s\n", 1, "qual")):
        with pytest.raises(rule.QtrimError) as e:
            rule.run(text)
        assert (e.value.code, e.value.record, e.value.kind) == (rule.ERR_UNSUPPORTED, record, kind)
    assert rule.run(good + b"@r\nAC\n+\nI@\n", phred_base=33)["rows"][1][0] == 2
    with pytest.raises(rule.QtrimError) as e:  # 'I' is a quality from '@' up, '?' is not
        rule.run(b"@r\nAC\n+\nI?\n", phred_base=64)
    assert e.value.kind == "qual"
    assert rule.run(good + b"\n\n\n")["out"] == good and rule.run(b"")["out"] == b""


# ------------------------------------------------------------------------------------- mk_fastq_pair_cuts
def _fastq(rng, reads, crlf=False, final_newline=True):
    nl = b"\r\n" if crlf else b"\n"
    out = []
    for i in range(reads):
        n = int(rng.integers(0, 40))
        out.append(b"@r%d" % i + nl + bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) + nl + b"+" + nl +
                   bytes(rng.integers(33, 74, n, dtype=np.uint8)) + nl)
    text = b"".join(out)
    return text if final_newline else text[:-len(nl)]


@pytest.mark.parametrize("crlf,final_newline", [(False, True), (True, True), (False, False), (True, False)])
def test_pair_cuts_fall_only_behind_even_records(crlf, final_newline):
    rng = np.random.default_rng(12)
    text = _fastq(rng, 61, crlf, final_newline)
    ends = np.cumsum([len(b"".join(r)) for r in rule.records(text)[0]]).tolist()
    behind_even = set(ends[1::2])
    for piece in (1, 7, 64, 100, 333, 1000, len(text), len(text) + 1):
        cuts = native.fastq_cuts(text, piece, pairs=True).tolist()
        assert cuts == rule.pair_cuts(text, piece)
        assert set(cuts) <= behind_even and all(0 < c < len(text) for c in cuts)
        bounds = [0] + cuts + [len(text)]
        assert all(b - a >= piece for a, b in zip(bounds[:-2], bounds[1:-1]))  # (only the last piece may be short)
    assert len(native.fastq_cuts(text, 1, pairs=True)) == 30 and len(native.fastq_cuts(text, 1)) == 60
    assert native.fastq_cuts(text, 1).tolist()[1::2] == native.fastq_cuts(text, 1, pairs=True).tolist()


def test_a_record_longer_than_the_piece_grows_its_piece():
    long_ = b"@l\n" + b"A" * 500 + b"\n+\n" + b"I" * 500 + b"\n"
    short = b"@s\nAC\n+\nII\n"
    text = short + long_ + short * 5 + long_ + short
    assert native.fastq_cuts(text, 100, pairs=True).tolist() == rule.pair_cuts(text, 100)
    cuts = rule.pair_cuts(text, 100)
    # the first pair alone passes 100 bytes; the next two pairs are 44 bytes together and grow by the pair with the long read
    assert cuts == [len(short + long_), 2 * len(short + long_) + 4 * len(short)]
    assert all((text[:c].count(b"\n") % 8) == 0 for c in cuts)
    assert native.fastq_cuts(b"", 5, pairs=True).tolist() == [] and native.fastq_cuts(short * 2, 1, pairs=True).tolist() == []
    assert native.fastq_cuts(short * 3, 1, pairs=True).tolist() == [2 * len(short)]
    assert native.fastq_cuts(short * 4, 1, pairs=True).tolist() == [2 * len(short)]


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


def test_header_declares_the_calls_and_the_version_stands():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ("mk_fastq_qtrim_text", "mk_fastq_qtrim_device", "mk_fastq_pair_cuts"):
        assert name in native.ABI_SYMBOLS and getattr(native.lib(), name) is not None
    args = re.search(r"int mk_fastq_qtrim_text\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "ctx", "fastq", "n", "piece_bytes", "opt", "cap", "keep", "rows", "hist", "out", "out_cap", "out_len", "nrec", "st"]
    args = re.search(r"int mk_fastq_qtrim_device\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "ctx", "d_fastq", "n", "opt", "cap", "d_keep", "d_rows", "d_hist", "d_out", "out_cap", "out_len", "nrec", "st"]
    assert len(native.lib().mk_fastq_qtrim_text.argtypes) == 14 and len(native.lib().mk_fastq_qtrim_device.argtypes) == 13
    args = re.search(r"int mk_fastq_pair_cuts\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["text", "n", "piece", "cuts", "cap", "ncuts"]
    assert "its quality line holds a character below the phred base" in HEADER
    assert native.MK_ABI == 6 and native.lib().mk_version().decode() == "mercat_hip 6.1 (gfx950)"


def test_bound_structs_match_the_header():
    fields = _struct_fields("mk_qtrim_opt_t")
    assert [f for _, f in fields] == ["phred_base", "cut_front", "cut_back", "min_len", "max_n", "low_q", "max_low_ppm", "min_mean_q",
                                      "paired", "which"]
    assert [(CTYPE[t], f) for t, f in fields] == [(t, f) for f, t in native.QtrimOpt._fields_] and C.sizeof(native.QtrimOpt) == 40
    fields = _struct_fields("mk_fastq_qtrim_t")
    assert [f for _, f in fields] == ["records", "records_out", "records_trimmed", "dropped_short", "dropped_n", "dropped_lowq",
                                      "dropped_meanq", "orphans", "bases_in", "bases_out", "bytes_out", "lines",
                                      "s_copy", "s_index", "s_scan", "s_place", "s_gather", "s_write"]
    assert [(CTYPE[t], f) for t, f in fields] == [(t, f) for f, t in native.FastqQtrim._fields_]
    assert [getattr(native.FastqQtrim, f).offset for _, f in fields] == [8 * i for i in range(18)] and C.sizeof(native.FastqQtrim) == 144
    st = native.FastqQtrim()
    st.dropped_n, st.s_scan = 3, 0.5
    assert st.as_dict()["dropped_n"] == 3 and st.as_dict()["s_scan"] == 0.5 and set(st.as_dict()) == {f for _, f in fields}


def test_python_layers_are_there():
    assert list(inspect.signature(native.Counter.fastq_qtrim).parameters)[1:] == [
        "path_or_bytes", "cut_back", "cut_front", "min_len", "max_n", "low_q", "max_low_frac", "min_mean_q", "phred_base", "paired",
        "which", "piece_bytes", "info"]
    d = {k: p.default for k, p in inspect.signature(native.Counter.fastq_qtrim).parameters.items()}
    assert (d["cut_back"], d["cut_front"], d["min_len"], d["max_n"], d["low_q"], d["max_low_frac"], d["min_mean_q"], d["phred_base"],
            d["paired"], d["which"], d["piece_bytes"], d["info"]) == (20, 0, 0, None, 0, 1.0, 0, 33, False, 1, 0, None)
    assert callable(native.Counter.fastq_qtrim_device)
    opt = native.qtrim_options(max_low_frac=0.25, max_n=None, paired=True, which=2)
    assert (opt.cut_back, opt.max_n, opt.max_low_ppm, opt.paired, opt.which) == (20, 0xFFFFFFFF, 250000, 1, 2)
    for bad in (dict(max_low_frac=1.5), dict(min_len=-1), dict(max_n=1 << 32)):
        with pytest.raises(ValueError):
            native.qtrim_options(**bad)
    names = list(inspect.signature(kmers.qtrim_reads).parameters)
    assert names[:2] == ["file", "out_path"] and {"tsv_path", "mate_file", "out_path2", "singles_path", "device"} <= set(names)
    assert "not fastp's" in kmers.qtrim_reads.__doc__
    with pytest.raises(ValueError):  # (before any call of the library)
        kmers.qtrim_reads("reads.fna", "out.fastq")
    assert kmers.fastq_names(b"@a b\nAC\n+\nII\n@c\nA\n+\nI") == ["a", "c"] and kmers.fastq_names(b"@a\nA\n+\nI\n\n\n") == ["a"]
    assert kmers.fastq_names(b"") == [] and kmers.fastq_names(b"@\n\n+\n\n") == [""]


def test_the_reports():
    got = rule.run(fq((b"ACGTAC", [30, 30, 30, 30, 2, 2]), (b"NN", [2, 2])), cut_back=20)
    tsv = report.format_qtrim_tsv(["r0", "r1"], got["rows"], got["keep"])
    assert tsv == b"record\tlength\tstart\tkept\tn\tlow\tqsum\tkeep\nr0\t6\t0\t4\t0\t0\t120\t1\nr1\t2\t0\t0\t0\t0\t0\t0\n"
    hist = [got["hist"][:256], got["hist"][256:]]
    text = report.format_qtrim_summary(got["figures"], hist)
    assert text == (b"metric\tbefore\tafter\nreads\t2\t1\nbases\t8\t4\nq20_bases\t4\t4\nq30_bases\t4\t4\nmean_quality\t16.0000\t30.0000\n"
                    b"dropped_short\t\t1\ndropped_n\t\t0\ndropped_lowq\t\t0\ndropped_meanq\t\t0\norphans\t\t0\n")
    with pytest.raises(ValueError):
        report.format_qtrim_tsv(["r0"], got["rows"], got["keep"])


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


def test_cli_accepts_qtrim(files):
    args = parse(files, ["-i", str(files / "r.fastq")], "-qtrim")
    assert args.qtrim == 20 and args.qtrim_front is None and not args.skipclean
    args = parse(files, ["-i", str(files / "s.fna"), str(files / "r.fastq")], "-qtrim", 25, "-qtrim_front", 10, "-qtrim_len", 30, "-qtrim_n", 0,
                 "-qtrim_low", 15, "-qtrim_low_frac", 0.4, "-qtrim_mean", 20, "-qtrim_phred", 64, "-skipclean")
    assert (args.qtrim, args.qtrim_front, args.qtrim_len, args.qtrim_n, args.qtrim_low, args.qtrim_low_frac, args.qtrim_mean,
            args.qtrim_phred) == (25, 10, 30, 0, 15, 0.4, 20, 64)
    assert parse(files, ["-f", str(files / "dir")], "-qtrim", 0).qtrim == 0
    assert cli.classify(files / "r.fastq", True) == ("nucleotide", "r")


def test_the_help_says_what_qtrim_is_not(capsys):
    with pytest.raises(SystemExit) as e:
        cli.parseargs(["-h"])
    help_ = " ".join(capsys.readouterr().out.split())
    assert e.value.code == 0 and "where MerCat2 runs fastp" in help_ and "not fastp's" in help_ and "-qtrim_phred" in help_


@pytest.mark.parametrize("extra,message", [
    (["-qtrim_front", 10], "-qtrim_front needs -qtrim"),
    (["-qtrim_len", 10], "-qtrim_len needs -qtrim"),
    (["-qtrim_n", 1], "-qtrim_n needs -qtrim"),
    (["-qtrim_low", 10], "-qtrim_low needs -qtrim"),
    (["-qtrim_low_frac", 0.5], "-qtrim_low_frac needs -qtrim"),
    (["-qtrim_mean", 10], "-qtrim_mean needs -qtrim"),
    (["-qtrim_phred", 64], "-qtrim_phred needs -qtrim"),
    (["-qtrim", 94], "-qtrim 94: must lie in 0..93"),
    (["-qtrim", -1], "-qtrim -1: must lie in 0..93"),
    (["-qtrim", "-qtrim_front", 94], "-qtrim_front 94: must lie in 0..93"),
    (["-qtrim", "-qtrim_len", -1], "-qtrim_len -1"),
    (["-qtrim", "-qtrim_n", -1], "-qtrim_n -1"),
    (["-qtrim", "-qtrim_low", 200], "-qtrim_low 200: must lie in 0..93"),
    (["-qtrim", "-qtrim_low", 10, "-qtrim_low_frac", 1.5], "-qtrim_low_frac 1.5: must lie in 0..1"),
    (["-qtrim", "-qtrim_low_frac", 0.5], "-qtrim_low_frac needs -qtrim_low"),
    (["-qtrim", "-qtrim_mean", 94], "-qtrim_mean 94: must lie in 0..93"),
    (["-qtrim", "-qtrim_phred", 50], "invalid choice"),
])
def test_cli_refuses(files, capsys, extra, message):
    with pytest.raises(SystemExit) as e:
        parse(files, ["-i", str(files / "r.fastq")], *extra)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_cli_refuses_qtrim_without_fastq_input(files, capsys):
    with pytest.raises(SystemExit) as e:
        parse(files, ["-i", str(files / "s.fna")], "-qtrim")
    assert e.value.code == 2 and "no input is a FASTQ file" in capsys.readouterr().err


def test_without_qtrim_the_refusal_stands(files):
    assert parse(files, ["-i", str(files / "r.fastq")]).qtrim is None
    with pytest.raises(SystemExit) as e:
        cli.classify(files / "r.fastq", False)
    assert str(e.value) == ("'r.fastq': without -skipclean MerCat2 trims FASTQ reads with fastp, which is not part of "
                            "this engine; -skipclean counts the reads untrimmed (fq2fa only), as MerCat2 does with "
                            "-skipclean or when fastp is not installed")
    assert cli.classify(files / "r.fastq", True) == ("nucleotide", "r") and cli.classify(files / "s.fna") == ("nucleotide", "s")
