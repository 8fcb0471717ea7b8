"""Host-side checks of the correction calls (mk_correct_text / mk_correct_device): the rule's hand examples against its
plain-Python restatement (tests/correct_rule.py), header, binding, report format and CLI layers.  No kernel is launched
here; tests/test_gpu_correct.py corrects on the GPU."""
import ctypes as C
import inspect
import random
import re

import numpy as np
import pytest

import correct_rule
from conftest import GOLDEN, ROOT
from mercat2_amd import cli, kmers, native, report

HEADER = (ROOT / "include" / "mercat_hip.h").read_text()
CTYPE = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int32_t": C.c_int32, "double": C.c_double}
READ = b"ACGGTCATTG"  # eight distinct 3-mers
SOLID = {READ[j:j + 3].decode(): 5 for j in range(8)}


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
    """(size, alignment, [(field, offset)]) of a header struct by the C rules."""
    at, align, fields = 0, 1, []
    for ctype, field in _struct_fields(name):
        size, al = (_layout(ctype)[:2] if ctype.startswith("mk_") else (C.sizeof(CTYPE[ctype]),) * 2)
        at = (at + al - 1) // al * al
        fields.append((field, at))
        at += size
        align = max(align, al)
    return (at + align - 1) // align * align, align, fields


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("a,b,windows,k,p", [
    (0, 7, 8, 3, None),     # the whole record
    (0, 0, 1, 3, None),     # ... of one window
    (0, 0, 8, 3, 0),        # at the start: p = b
    (0, 1, 8, 3, 1),
    (0, 2, 8, 3, 2),        # n == k at the start
    (0, 3, 8, 3, None),     # n == k + 1 at the start
    (7, 7, 8, 3, 9),        # at the end: p = a + k - 1
    (6, 7, 8, 3, 8),
    (5, 7, 8, 3, 7),        # n == k at the end
    (4, 7, 8, 3, None),     # n == k + 1 at the end
    (2, 4, 8, 3, 4),        # interior, n == k
    (2, 3, 8, 3, None),     # interior, n == k - 1
    (2, 5, 8, 3, None),     # interior, n == k + 1
    (1, 1, 3, 1, 1),        # k = 1: the window is the base
])
def test_shape_table(a, b, windows, k, p):
    assert correct_rule.candidate_of(a, b, windows, k) == p


def test_runs_of():
    T, F = True, False
    assert correct_rule.runs_of([]) == [] and correct_rule.runs_of([F, F]) == []
    assert correct_rule.runs_of([T, F, T, T, F, F, T]) == [(0, 0), (2, 3), (6, 6)]
    assert correct_rule.runs_of([T, T, T]) == [(0, 2)]


@pytest.mark.parametrize("seq,table,out,row", [
    (b"ACGGACATTG", SOLID, READ, (1, 1, 0, 0)),                          # interior: windows 2..4, p = 4, only T repairs
    (b"CCGGTCATTG", SOLID, READ, (1, 1, 0, 0)),                          # position 0
    (b"ACTGTCATTG", SOLID, READ, (1, 1, 0, 0)),                          # position k - 1: n == k at the start
    (b"ACGGTCAATG", SOLID, READ, (1, 1, 0, 0)),                          # position L - k: n == k at the end
    (b"ACGGTCATTC", SOLID, READ, (1, 1, 0, 0)),                          # position L - 1
    (b"CCGGTCATTC", SOLID, READ, (2, 2, 0, 0)),                          # both ends
    (b"GGGGG", SOLID, b"GGGGG", (1, 0, 0, 0)),                           # nothing solid: no candidate
    (READ, dict(SOLID, GGT=1, GTC=1), READ, (1, 0, 0, 0)),               # interior, n == k - 1
    (READ, dict(SOLID, GGT=1, GTC=1, TCA=1, CAT=1), READ, (1, 0, 0, 0)),  # interior, n == k + 1
    (READ, dict(SOLID, ACG=1, CGG=1, GGT=1, GTC=1), READ, (1, 0, 0, 0)),  # at the start, n == k + 1
    (READ, SOLID, READ, (0, 0, 0, 0)),
    (b"AC", SOLID, b"AC", (0, 0, 0, 0)),                                 # no window
    (b"GCGGT", {"ACG": 5, "TCG": 5, "CGG": 5, "GGT": 5}, b"GCGGT", (1, 0, 1, 0)),  # A and T both repair
    (b"GCGGT", {"CGG": 5, "GGT": 5}, b"GCGGT", (1, 0, 0, 1)),            # nothing repairs
    (b"ACGGNCATTG", SOLID, READ, (1, 1, 0, 0)),                          # an N at p: four alternatives, one viable
    (b"ACGGNCATTG", dict(SOLID, GGA=5, GAC=5, ACA=5), b"ACGGNCATTG", (1, 0, 1, 0)),  # ... two viable: A counts as one
    (b"ACGGtCATTG", dict(SOLID, GGA=5, GAC=5, ACA=5), b"ACGGtCATTG", (1, 0, 1, 0)),  # a lower-case base is no base
    (b"ACGGTCATTG", dict(SOLID, GGT=1, GTC=1, TCA=1, GGA=5, GAC=5, ACA=5), b"ACGGACATTG", (1, 1, 0, 0)),  # T is not its own alternative
])
def test_hand_examples(seq, table, out, row):
    assert correct_rule.correct_seq(seq, table, 3, 2) == (out, row)


def test_text_and_output():
    # a headless start, a wrapped CR LF record with a '*', a header alone, a record shorter than k, no last newline
    text = b"ACGGACATTG\n>r x\r\nCCGG\r\nTCA*TTG\r\n>h\n  >s\rAC\r>last\nACGGTCATTC"
    out, rows = correct_rule.expected(text, SOLID, 3, 2)
    assert out == b"ACGGTCATTG\n>r x\r\nACGGTCATTG\n>h\n  >s\rAC\n>last\nACGGTCATTG\n"
    assert rows == [(1, 1, 0, 0), (1, 1, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0), (1, 1, 0, 0)]
    assert len(out) <= len(text) + 1
    # a header line without a terminator is the whole record
    assert correct_rule.expected(b">a\nACG\n>end", SOLID, 3, 2)[0] == b">a\nACG\n>end"
    # one-line LF records in which nothing is fixed come back byte for byte; at_least 1: only an absent k-mer is weak
    whole = b">a\nACGGTCATTG\n>b\nGGGGG\n>c\n"
    assert correct_rule.expected(whole, SOLID, 3, 2)[0] == whole
    assert correct_rule.expected(b">a\nACGGTCATTG\n", dict(SOLID, GGT=1), 3, 1) == (b">a\nACGGTCATTG\n", [(0, 0, 0, 0)])
    # fold: the windows count under min(window, reverse complement)
    folded = {min(key, key.translate(str.maketrans("ACGT", "TGCA"))[::-1]): 5 for key in SOLID}
    rc = READ.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]
    bad = rc[:4] + b"A" + rc[5:]
    assert rc[4:5] != b"A" and correct_rule.correct_seq(bad, folded, 3, 2, fold=True) == (rc, (1, 1, 0, 0))
    assert correct_rule.correct_seq(bad, folded, 3, 2, fold=False)[0] == bad


def _read(seed, k, length):
    rng = random.Random(seed)
    while True:
        s = "".join(rng.choice("ACGT") for _ in range(length)).encode()
        if len({s[j:j + k] for j in range(length - k + 1)}) == length - k + 1:
            return s


def _sub(seq, *at):
    out = bytearray(seq)
    for p in at:
        out[p] = b"ACGT"[(b"ACGT".index(out[p]) + 1 + p % 3) % 4]
    return bytes(out)


@pytest.mark.parametrize("k", [11, 21, 31])  # (long enough that no substituted window is another window of the read)
def test_substitutions_in_a_read_of_distinct_kmers(k):
    L = 4 * k + 7
    seq = _read(k, k, L)
    table = {seq[j:j + k].decode(): 3 for j in range(L - k + 1)}
    for p in (0, k - 1, k, L - k, L - 1, L // 2):
        bad = _sub(seq, p)
        assert bad != seq and correct_rule.correct_seq(bad, table, k, 2) == (seq, (1, 1, 0, 0)), p
    # two substitutions k - 1 and k apart make one run longer than k; k + 1 apart, two runs of k with a solid window between
    at = k + 2
    for gap in (k - 1, k):
        bad = _sub(seq, at, at + gap)
        assert correct_rule.correct_seq(bad, table, k, 2) == (bad, (1, 0, 0, 0)), gap
    assert correct_rule.correct_seq(_sub(seq, at, at + k + 1), table, k, 2) == (seq, (2, 2, 0, 0))
    assert correct_rule.correct_seq(_sub(seq, 0, at, at + k + 1, L - 1), table, k, 2) == (seq, (4, 4, 0, 0))


def _one_at_a_time(seq, table, k, at_least, last_first):
    """Fix one run, derive the runs again, fix the next -- until no run of the record can be fixed."""
    while True:
        weak = correct_rule.weak_of(seq, table, k, at_least, False)
        fixable = []
        for i, (a, b) in enumerate(correct_rule.runs_of(weak)):
            p = correct_rule.candidate_of(a, b, len(weak), k)
            if p is not None and len(correct_rule.judge(seq, a, b, p, table, k, at_least, False)) == 1:
                fixable.append(i)
        if not fixable:
            return seq
        seq = correct_rule.correct_seq(seq, table, k, at_least, only=fixable[-1 if last_first else 0])[0]


@pytest.mark.parametrize("k", [11, 31])
def test_the_order_of_the_fixes_reaches_nothing(k):
    L = 6 * k
    seq = _read(2 * k, k, L)
    table = {seq[j:j + k].decode(): 3 for j in range(L - k + 1)}
    bad = _sub(seq, 0, k + 1, 2 * k + 2, 3 * k + 3, 3 * k + 3 + k - 1, L - 1)  # four fixable runs and one that is too long
    at_once, row = correct_rule.correct_seq(bad, table, k, 2)
    assert row == (5, 4, 0, 0) and at_once != seq and at_once == _sub(seq, 3 * k + 3, 3 * k + 3 + k - 1)
    assert _one_at_a_time(bad, table, k, 2, False) == at_once == _one_at_a_time(bad, table, k, 2, True)


# ---------------------------------------------------------------------------------------------- the header
def test_header_declares_the_calls_and_flags():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ("mk_correct_text", "mk_correct_device"):
        assert re.search(r"\bint %s\s*\(mk_ctx\*" % name, code)
        assert name in native.ABI_SYMBOLS and getattr(native.lib(), name) is not None
    assert re.search(r"#define MK_CORRECT_FOLD\s+1u", code)
    assert native.CORRECT_FOLD == native.SCREEN_FOLD == 1
    args = re.search(r"int mk_correct_text\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "ctx", "text", "n", "piece_bytes", "flags", "rule", "out", "out_cap", "out_len", "fix", "rows", "cap", "nrows", "st"]
    assert "const mk_correct_rule_t* rule" in args and "mk_correct_row_t* fix" in args
    args = re.search(r"int mk_correct_device\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "ctx", "d_text", "n", "flags", "rule", "d_out", "out_cap", "out_len", "d_fix", "d_rows", "cap", "nrows", "st"]
    assert len(native.lib().mk_correct_text.argtypes) == 14 and len(native.lib().mk_correct_device.argtypes) == 13
    assert native.MK_ABI == 6 and native.lib().mk_version().decode().split()[1].split(".")[0] == "6"


def test_bound_structs_match_the_header():
    want_size, _, want = _layout("mk_correct_t")
    assert [f for f, _ in want] == [g[0] for g in native.Correct._fields_]
    assert [(f, getattr(native.Correct, f).offset) for f, _ in want] == want
    assert C.sizeof(native.Correct) == want_size == 96 + 9 * 8 + 6 * 8
    for (ctype, field), (_, got) in zip(_struct_fields("mk_correct_t"), native.Correct._fields_):
        assert got is (native.Screen if ctype == "mk_screen_t" else CTYPE[ctype]), field
    assert [f for _, f in _struct_fields("mk_correct_t")] == [
        "screen", "records", "runs", "candidates", "fixed", "ambiguous", "unfixable", "bases", "bytes_out", "preamble",
        "s_place", "s_track", "s_runs", "s_try", "s_gather", "s_write"]
    want_size, _, want = _layout("mk_correct_rule_t")
    assert want == [("at_least", 0), ("reserved", 8)] and C.sizeof(native.CorrectRule) == want_size == 16
    assert [(f, getattr(native.CorrectRule, f).offset) for f, _ in native.CorrectRule._fields_] == want
    want_size, _, want = _layout("mk_correct_row_t")
    assert want == [("runs", 0), ("fixed", 4), ("ambiguous", 8), ("unfixable", 12)] and want_size == 16
    assert native.CorrectRow.itemsize == 16 and native.CorrectRow.names == native.CORRECT_COLUMNS == tuple(f for f, _ in want)
    assert [native.CorrectRow.fields[f][1] for f, _ in want] == [at for _, at in want]
    fix = np.arange(8, dtype=np.uint32).reshape(2, 4)
    assert fix.view(native.CorrectRow)["ambiguous"].ravel().tolist() == [2, 6]
    st = native.Correct()
    st.screen.records, st.runs, st.fixed, st.s_try = 7, 5, 3, 0.5
    d = st.as_dict()
    assert d["records"] == 0 and d["runs"] == 5 and d["fixed"] == 3 and d["s_try"] == 0.5  # (mk_correct_t's own records)
    assert {"candidates", "ambiguous", "unfixable", "bases", "bytes_out", "preamble", "s_place", "s_track", "s_runs", "s_gather",
            "s_write", "s_probe", "pieces"} <= set(d)


def test_python_layers_are_there():
    for name in ("correct", "correct_device"):
        assert callable(getattr(native.Counter, name))
    sig = inspect.signature(native.Counter.correct).parameters
    assert list(sig)[1:] == ["path_or_bytes", "at_least", "fold", "piece_bytes", "info"] and sig["at_least"].default == 2
    sig = inspect.signature(kmers.correct_reads).parameters
    assert list(sig) == ["table", "file", "out_path", "at_least", "rounds", "tsv_path", "mate_file", "out_path2"]
    assert sig["at_least"].default == 2 and sig["rounds"].default == 1
    assert "FASTQ" in kmers.correct_reads.__doc__ and "fq2fa" in kmers.correct_reads.__doc__
    assert callable(report.write_correct_tsv)
    with pytest.raises(ValueError):
        kmers.correct_reads(None, "x.fa", "y.fa", rounds=0)
    with pytest.raises(ValueError):
        kmers.correct_reads(None, "x.fa", "y.fa", out_path2="z.fa")


# ----------------------------------------------------------------------------------------------- the report
def test_correct_tsv_format(tmp_path):
    names = ["r1", "", "clean"]
    lengths = [150, 18446744073709551615, 20]
    fix = np.array([[3, 1, 1, 0], [4294967295, 4294967295, 0, 0], [0, 0, 0, 0]], dtype=np.uint32)
    want = (b"record\tlength\truns\tfixed\tambiguous\tunfixable\nr1\t150\t3\t1\t1\t0\n"
            b"\t18446744073709551615\t4294967295\t4294967295\t0\t0\nclean\t20\t0\t0\t0\t0\n")
    assert report.write_correct_tsv(tmp_path / "t.tsv", names, lengths, fix) == 3 and (tmp_path / "t.tsv").read_bytes() == want
    assert report.format_correct_tsv(names, lengths, [tuple(r) for r in fix.tolist()]) == want
    assert report.format_correct_tsv([], [], fix[:0]) == b"record\tlength\truns\tfixed\tambiguous\tunfixable\n"
    with pytest.raises(ValueError):
        report.write_correct_tsv(tmp_path / "x.tsv", names, lengths, fix[:2])
    with pytest.raises(ValueError):
        report.format_correct_tsv(names, lengths[:2], fix)


# -------------------------------------------------------------------------------------------------- the CLI
def test_cli_accepts(tmp_path):
    fasta = str(GOLDEN / "inputs" / "A.fasta")
    args, _ = cli.parseargs(["-i", fasta, "-k", "5", "-correct", fasta])
    assert (args.correct, args.correct_kind, args.correct_min, args.correct_rounds, args.correct_mate) == (fasta, "nucleotide", 2, 1, None)
    args, _ = cli.parseargs(["-i", fasta, "-k", "64", "-correct", fasta, "-correct_min", "3", "-correct_rounds", "2", "-correct_mate", fasta])
    assert (args.correct_min, args.correct_rounds, args.correct_mate) == (3, 2, fasta)
    for name in ("x.fastq.gz", "x.fq", "x.fna", "x.fa.gz"):
        (tmp_path / name).write_bytes(b"")
        assert cli.parseargs(["-i", fasta, "-k", "5", "-correct", str(tmp_path / name)])[0].correct_kind == "nucleotide"
    args, _ = cli.parseargs(["-i", fasta, "-k", "5"])
    assert args.correct is None and args.correct_kind is None and args.correct_min is None and args.correct_rounds is None


def test_cli_rejects(tmp_path, capsys):
    fasta = str(GOLDEN / "inputs" / "A.fasta")
    (tmp_path / "p.faa").write_bytes(b">p\nMKV\n")
    out = tmp_path / "out"
    for extra in (["-correct", str(tmp_path / "missing.fa")], ["-correct", str(ROOT / "README.md")], ["-correct_min", "2"],
                  ["-correct_rounds", "2"], ["-correct_mate", fasta], ["-correct", fasta, "-correct_min", "0"],
                  ["-correct", fasta, "-correct_min", "-1"], ["-correct", fasta, "-correct_rounds", "0"],
                  ["-correct", fasta, "-correct_min", "x"], ["-correct", str(tmp_path / "p.faa")],
                  ["-correct", fasta, "-correct_mate", str(tmp_path / "missing.fa")],
                  ["-correct", fasta, "-correct_mate", str(tmp_path / "p.faa")]):
        with pytest.raises(SystemExit) as e:
            cli.main(["-i", fasta, "-k", "5", "-o", str(out)] + extra)
        assert e.value.code == 2 and not out.exists(), extra  # (before the output folder is made, before any counting)
    with pytest.raises(SystemExit) as e:
        cli.main(["-i", fasta, "-k", "65", "-o", str(out), "-correct", fasta])
    assert e.value.code == 2 and not out.exists()
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        cli.main(["-i", fasta, "-k", "5", "-o", str(out), "-correct", str(tmp_path / "p.faa")])
    assert "protein" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        cli.parseargs(["-h"])
    text = " ".join(capsys.readouterr().out.split())
    assert e.value.code == 0 and "-correct FILE" in text and "-correct_min" in text and "-correct_rounds" in text and \
        "-correct_mate" in text and "_corrected.fna" in text
