"""What can be checked of the ORF calls without a GPU: the rule itself (tests/orf_rule.py) on examples written out by
hand, on a property and on prodigal's own calls for a slice of a real genome; the header text, the bindings, the TSV
writer and the CLI's refusals; the kernel's tile span."""
import ctypes
import random
import re

import pytest

import orf_rule as rule
from conftest import GOLDEN, ROOT
from mercat2_amd import cli, native, report

HEADER = (ROOT / "include" / "mercat_hip.h").read_text()
SOURCE = (ROOT / "mercat2_amd" / "csrc" / "mk_orf.hip").read_text()


def test_codon_table_in_both_spellings():
    """The table in A C G T order (the kernel's index 16 c1 + 4 c2 + c3) is NCBI table 1, which NCBI prints in T C A G
    order."""
    assert rule.CODON_TABLE == "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"
    assert rule.NCBI_TABLE_1 == "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
    assert native.CODON_TABLE == rule.CODON_TABLE
    assert re.search(r'OR_TABLE\[65\] = "([A-Z*]{64})"', SOURCE).group(1) == rule.CODON_TABLE
    assert rule.CODON_TABLE in HEADER
    tcag = "TCAG"
    for i, a in enumerate("ACGT"):
        for j, b in enumerate("ACGT"):
            for k, c in enumerate("ACGT"):
                assert rule.CODON_TABLE[16 * i + 4 * j + k] == rule.NCBI_TABLE_1[16 * tcag.index(a) + 4 * tcag.index(b) + tcag.index(c)]
    stops = [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT" if rule.translate(rule.codes((a + b + c).encode())) == "*"]
    assert sorted(stops) == sorted(rule.STOPS) == ["TAA", "TAG", "TGA"]
    assert rule.translate(rule.codes(b"ATG")) == "M" and rule.translate(rule.codes(b"auG")) == "M" and rule.translate(rule.codes(b"ANG")) == "X"


HAND = b">rec1 first record\nATGAAATAAGG\r\nCcat\n>only_header\n>r2\tx\nnnATGuGACC\nTTA\n"


def test_hand_example():
    """rec1 = ATGAAATAAGGCcat (wrapped, CR LF, lowercase), a header-only record, r2 = nnATGuGACCTTA (N codons, U).
    rec1 forward: frame 1 ATG AAA TAA GGC cat = M K * G H, frame 2 TGA AAT AAG GCc = * N K A, frame 3 GAA ATA AGG Cca =
    E I R P; its reverse complement ATGGCCTTATTTCAT: MALFH, W P Y F, G L I S.  Ordered by the right end: 6 (MK), 13 (NKA,
    then the reverse GLIS), 14, 15."""
    assert rule.records(HAND) == [(b"rec1", b"ATGAAATAAGGCcat"), (b"only_header", b""), (b"r2", b"nnATGuGACCTTA")]
    out, rows = rule.expected(HAND, 2)
    assert out == (b">rec1_1_1_1\nMK\n>rec1_5_2_2\nNKA\n>rec1_2_6_3\nGLIS\n>rec1_3_3_4\nEIRP\n>rec1_3_5_5\nWPYF\n>rec1_10_1_6\nGH\n"
                   b">rec1_1_4_7\nMALFH\n>r2_2_4_1\nGHX\n>r2_3_6_2\nRSH\n>r2_1_1_3\nXCDL\n>r2_1_5_4\nKVTX\n>r2_2_2_5\nXVTL\n")
    assert rows == [[0, 0, 2, 1], [0, 4, 3, 2], [0, 1, 4, 6], [0, 2, 4, 3], [0, 2, 4, 5], [0, 9, 2, 1], [0, 0, 5, 4],
                    [2, 1, 3, 4], [2, 2, 3, 6], [2, 0, 4, 1], [2, 0, 4, 5], [2, 1, 4, 2]]
    # the strand flags: ranks count what is emitted
    assert rule.expected(HAND, 2, strand="plus")[0] == (b">rec1_1_1_1\nMK\n>rec1_5_2_2\nNKA\n>rec1_3_3_3\nEIRP\n>rec1_10_1_4\nGH\n"
                                                       b">r2_1_1_1\nXCDL\n>r2_2_2_2\nXVTL\n")
    assert rule.expected(HAND, 2, strand="minus")[0] == (b">rec1_2_6_1\nGLIS\n>rec1_3_5_2\nWPYF\n>rec1_1_4_3\nMALFH\n"
                                                        b">r2_2_4_1\nGHX\n>r2_3_6_2\nRSH\n>r2_1_5_3\nKVTX\n")
    # start mode: MK and MALFH begin with their ATG; in r2 nnA TGu GAC ... holds ATG only in frame 3, in front of uGA
    assert rule.expected(HAND, 1, start=True) == (b">rec1_1_1_1\nMK\n>rec1_1_4_2\nMALFH\n>r2_3_3_1\nM\n", [[0, 0, 2, 1], [0, 0, 5, 4], [2, 2, 1, 3]])
    assert rule.expected(HAND, 1, start=True, alt_starts=True)[0] == b">rec1_1_1_1\nMK\n>rec1_1_4_2\nMALFH\n>r2_3_3_1\nM\n>r2_5_2_2\nVTL\n"
    # a headless record has the empty name; ATG AAA = M K ends at 6, frame 2 is TGA, frame 3 GAA = E ends at 5
    assert rule.expected(b"ATGAAA\n>x\nAT\n", 1, strand="plus")[0] == b">_3_3_1\nE\n>_1_1_2\nMK\n"


def test_start_mode_by_hand():
    # two ATG in one forward stretch: the first starts the ORF
    assert rule.expected(b">f\nCCATGCCCATGCCTAACC\n", 1, start=True, strand="plus") == (b">f_3_3_1\nMPMPN\n", [[0, 2, 5, 3]])
    # two CAT in one reverse stretch, at 2 and 8: the rightmost is the first the reverse strand reads; [2, 11) = M G M
    assert rule.expected(b">m\nCCCATCCCCATCC\n", 1, start=True, strand="minus") == (b">m_3_6_1\nMGM\n", [[0, 2, 3, 6]])
    assert rule.expected(b">m\nCCCATCCCCATCC\n", 1, strand="minus")[0] == b">m_3_6_1\nMGM\n>m_1_5_2\nDGDG\n>m_2_4_3\nGWGW\n"
    # GTG and TTG start with alt_starts only, and are translated as they stand
    text = b">a\nCCGTGCCTTGCCATGCC\n"
    assert rule.expected(text, 1, start=True, strand="plus")[0] == b">a_13_1_1\nM\n"
    assert rule.expected(text, 1, start=True, alt_starts=True, strand="plus")[0] == b">a_13_1_1\nM\n>a_8_2_2\nLPC\n>a_3_3_3\nVPCHA\n"
    # a stretch without a start yields nothing
    assert rule.expected(b">n\n" + b"GCC" * 40 + b"\n", 1, start=True) == (b"", [])


def test_the_96_base_boundary():
    # 97 bases: [0, 96) is class 0 forward and class 1 of the reverse strand, [1, 97) class 1 forward and class 0 reverse
    for n, want in ((95, []), (96, [1, 4]), (97, [1, 5, 2, 4])):
        out, rows = rule.expected(b">r\n" + (b"GC" * 60)[:n] + b"\n", 32)
        assert [r[3] for r in rows] == want and all(r[2] == 32 for r in rows)
    assert len(rule.expected(b">r\n" + b"G" * 95 + b"\n", 31)[1]) == 6


def test_every_stretch_is_one_orf():
    rng = random.Random(3)
    for trial in range(20):
        seq = "".join(rng.choice("ACGTACGTN") for _ in range(rng.randrange(0, 700)))
        min_aa = rng.choice((1, 5, 20))
        got = rule.record_orfs(seq.encode(), min_aa)
        by_class = {}
        for begin, aa, frame, aas in got:
            assert aa == len(aas) >= min_aa and "*" not in aas
            by_class.setdefault(frame, []).append((begin, begin + 3 * aa))
        comp = seq.translate(str.maketrans("ACGT", "TGCA"))[::-1]
        for frame, spans in by_class.items():
            spans.sort()
            for (a0, b0), (a1, b1) in zip(spans, spans[1:]):  # never two that touch without a stop between them
                assert b0 + 3 <= a1
                if frame < 4:  # a forward ORF that is not the record's last ends in front of a stop
                    assert seq[b0:b0 + 3] in rule.STOPS
                else:  # a reverse ORF that is not the record's first begins behind one (TTA CTA TCA read forward)
                    assert seq[a1 - 3:a1] in ("TTA", "CTA", "TCA")
        # every stretch of at least min_aa codons is there: count them with a regular expression over the translation
        for strand, s in ((0, seq), (1, comp)):
            for c in range(3):
                prot = "".join(rule.translate(rule.codes(s[i:i + 3].encode())) for i in range(c, len(s) - 2, 3))
                want = [m for m in re.findall(r"[^*]+", prot) if len(m) >= min_aa]
                have = [aas for _, _, frame, aas in got if frame == (4 if strand else 1) + c]
                assert sorted(want) == sorted(have)


def test_prodigal_calls_are_found():
    """The first 24 000 bases of the reference's RW1.fna and the 22 proteins prodigal calls in them
    (tests/golden/orf/README.md): no tolerance."""
    text = (GOLDEN / "orf" / "RW1_24k.fna").read_bytes()
    prots = rule.proteins((GOLDEN / "orf" / "RW1_24k_pro.faa").read_bytes())
    assert len(prots) == 22 and len(rule.records(text)[0][1]) == 24000

    def seqs(**mode):
        return [line for line in rule.expected(text, 20, **mode)[0].decode().split("\n") if line and not line.startswith(">")]

    stop, start, alt = seqs(), seqs(start=True), seqs(start=True, alt_starts=True)
    assert sum(any(s.endswith(p[1:]) for s in stop) for _, p in prots) == 22  # behind the first residue
    whole = [p for h, p in prots if "partial=00" in h and "start_type=ATG" in h]
    assert len(whole) == 16 and sum(any(s.endswith(p) for s in start) for p in whole) == 16
    complete = [p for h, p in prots if "partial=00" in h]
    assert len(complete) == 21 and sum(any(s.endswith(p[1:]) for s in alt) for p in complete) == 21
    assert len(rule.expected(text, 32)[1]) == 265


def test_header_and_bindings():
    for word in ("#define MK_ORF_START 1u", "#define MK_ORF_ALT   2u", "#define MK_ORF_PLUS  4u", "#define MK_ORF_MINUS 8u",
                 "typedef struct mk_orf_opt_t { uint32_t min_aa, flags; } mk_orf_opt_t;",
                 "typedef struct mk_orf_row_t { uint64_t record, begin; uint32_t aa, frame; } mk_orf_row_t;",
                 "uint64_t bytes, records, bases, orfs, residues, bytes_out, longest, per_frame[6], preamble;",
                 "int32_t headless, pieces;", "double s_read, s_parse, s_find, s_place, s_emit, s_write, s_total;",
                 "int mk_orf_text  (mk_ctx*", "int mk_orf_device(mk_ctx*"):
        assert word in HEADER, word
    assert "#define MK_ABI 6" in HEADER or native.MK_ABI == 6
    assert (native.ORF_START, native.ORF_ALT, native.ORF_PLUS, native.ORF_MINUS) == (1, 2, 4, 8)
    assert native.ORF_ROW_DTYPE.itemsize == 24 and ctypes.sizeof(native.OrfOpt) == 8
    assert ctypes.sizeof(native.Orf) == 14 * 8 + 2 * 4 + 7 * 8
    assert [n for n, _ in native.Orf._fields_] == ["bytes", "records", "bases", "orfs", "residues", "bytes_out", "longest", "per_frame",
                                                  "preamble", "headless", "pieces", "s_read", "s_parse", "s_find", "s_place", "s_emit",
                                                  "s_write", "s_total"]
    assert "mk_orf_text" in native.ABI_SYMBOLS and "mk_orf_device" in native.ABI_SYMBOLS
    opt = native.orf_options(20, True, True, "minus")
    assert (opt.min_aa, opt.flags) == (20, 1 | 2 | 8) and native.orf_options().flags == 0 and native.orf_options().min_aa == 32
    for bad in (dict(alt_starts=True), dict(strand="up"), dict(min_aa=-1), dict(min_aa=1 << 32)):
        with pytest.raises(ValueError):
            native.orf_options(**bad)


def test_library_exports_the_calls():
    L = native.lib()
    assert L.mk_orf_text and L.mk_orf_device


def test_format_orf_tsv(tmp_path):
    rows = [[0, 0, 2, 1], [0, 1, 4, 6], [2, 9, 33, 3]]
    want = b"record\tname\tbegin\tend\tstrand\tframe\taa\n0\trec1\t0\t6\t+\t1\t2\n0\trec1\t1\t13\t-\t6\t4\n2\t\xc3\xa9\t9\t108\t+\t3\t33\n"
    assert report.format_orf_tsv([b"rec1", b"", b"\xc3\xa9"], rows) == want
    assert report.format_orf_tsv(["rec1", "", "é"], rows) == want
    assert report.write_orf_tsv(tmp_path / "o.tsv", [b"rec1", b"", b"\xc3\xa9"], rows) == 3 and (tmp_path / "o.tsv").read_bytes() == want
    assert report.format_orf_tsv([], []) == b"record\tname\tbegin\tend\tstrand\tframe\taa\n"
    with pytest.raises(ValueError):
        report.format_orf_tsv([b"a"], [[1, 0, 1, 1]])


def test_cli_refusals(tmp_path, capsys):
    (tmp_path / "a.fna").write_text(">a\nACGT\n")
    (tmp_path / "p.faa").write_text(">p\nMKV\n")
    (tmp_path / "a_orf.faa").write_text(">p\nMKV\n")
    base = ["-k", "3", "-o", str(tmp_path / "out")]

    def refused(argv, word):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err
        assert not (tmp_path / "out").exists()  # before anything runs

    refused(["-i", str(tmp_path / "p.faa"), "-orf"] + base, "no nucleotide input")
    refused(["-i", str(tmp_path / "a.fna"), str(tmp_path / "a_orf.faa"), "-orf"] + base, "a_orf")
    refused(["-i", str(tmp_path / "a.fna"), "-orf", "-orf_alt"] + base, "-orf_alt needs -orf_start")
    refused(["-i", str(tmp_path / "a.fna"), "-orf_start"] + base, "need -orf")
    refused(["-i", str(tmp_path / "a.fna"), "-orf", "0"] + base, "MIN_AA")
    refused(["-i", str(tmp_path / "a.fna"), "-prod"] + base, "not part of this engine")
    args, _ = cli.parseargs(["-i", str(tmp_path / "a.fna"), "-orf"] + base)
    assert args.orf == 32 and not args.orf_start and args.orf_strand is None
    args, _ = cli.parseargs(["-i", str(tmp_path / "a.fna"), "-orf", "20", "-orf_start", "-orf_alt", "-orf_strand", "minus"] + base)
    assert (args.orf, args.orf_start, args.orf_alt, args.orf_strand) == (20, True, True, "minus")


def test_tile_span_of_the_kernel():
    import test_gpu_orf
    run = int(re.search(r"^#define OR_RUN (\d+)\b", SOURCE, re.M).group(1))
    assert re.search(r"^#define OR_SPAN \(256 \* OR_RUN\)", SOURCE, re.M)
    assert (test_gpu_orf.RUN, test_gpu_orf.SPAN) == (run, 256 * run) and run % 3 == 0 and run % 16 == 0
