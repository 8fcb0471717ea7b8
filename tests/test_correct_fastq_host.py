"""mk_correct_fastq_* without a GPU: the rule in plain Python (tests/correct_fastq_rule.py) on hand examples and
against the FASTA rule through fq2fa, the struct layouts, the Python layers' signatures, the ValueErrors and every CLI
refusal.  Nothing here opens a context."""
import ctypes as C
import inspect
import random

import pytest

import correct_fastq_rule as cfr
import correct_rule
import fastq_select_rule as fsr
import trim_rule
from mercat2_amd import cli, kmers, native

K = 5
CLEAN = b"ACGTTGCAAGGCTTAGACCGATATCGGA"  # every 5-mer once


def table_of(*seqs, k=K, count=2):
    return {s[j:j + k].decode(): count for s in seqs for j in range(len(s) - k + 1)}


def sub(seq, *at):
    out = bytearray(seq)
    for p in at:
        out[p] = b"CGTA"[b"ACGT".index(out[p])]
    return bytes(out)


TABLE = table_of(CLEAN)
assert len(TABLE) == len(CLEAN) - K + 1
BAD = sub(CLEAN, 12)
QUAL = bytes(33 + (i % 40) for i in range(len(CLEAN)))


# ------------------------------------------------------------------------------------------------- the rule
def test_rule_fixes_the_base_and_keeps_every_other_byte():
    text = b"@r1 x\n" + BAD + b"\n+\n" + QUAL + b"\n"
    out, rows = cfr.expected(text, TABLE, K, 2)
    assert out == b"@r1 x\n" + CLEAN + b"\n+\n" + QUAL + b"\n" and rows == [(1, 1, 0, 0)]
    out, _ = cfr.expected(text, TABLE, K, 2, new_qual=ord("!"))
    q = bytearray(QUAL)
    q[12] = ord("!")
    assert out == b"@r1 x\n" + CLEAN + b"\n+\n" + bytes(q) + b"\n"
    assert cfr.figures(text, rows) == {"lines": 4, "records": 1, "patched": 1, "fixed": 1, "bytes_out": len(text), "runs": 1,
                                       "ambiguous": 0, "unfixable": 0}


@pytest.mark.parametrize("first", [b"@", b">", b"+"])
def test_rule_quality_line_may_start_with_anything(first):
    qual = first + QUAL[1:]
    text = b"@a\n" + BAD + b"\n+\n" + qual + b"\n@b\n" + CLEAN + b"\n+\n" + qual + b"\n"
    out, rows = cfr.expected(text, TABLE, K, 2, new_qual=ord("I"))
    q = bytearray(qual)
    q[12] = ord("I")
    assert out == b"@a\n" + CLEAN + b"\n+\n" + bytes(q) + b"\n@b\n" + CLEAN + b"\n+\n" + qual + b"\n"
    assert rows == [(1, 1, 0, 0), (0, 0, 0, 0)]


def test_rule_layouts_keep_their_bytes():
    plus = b"+a name that is longer than the read " + b"x" * 40
    crlf = b"@c d\r\n" + BAD + b"\r\n" + plus + b"\r\n" + QUAL + b"\r\n"
    out, rows = cfr.expected(crlf, TABLE, K, 2)
    assert out == crlf.replace(BAD, CLEAN) and rows == [(1, 1, 0, 0)]
    open_last = b"@e\n\n+\n\n@o\n" + BAD + b"\n+\n" + QUAL  # (L = 0 in front, no final newline)
    out, rows = cfr.expected(open_last, TABLE, K, 2)
    assert out == open_last.replace(BAD, CLEAN) and not out.endswith(b"\n") and rows == [(0, 0, 0, 0), (1, 1, 0, 0)]
    for extra in (b"\n", b"\n\n", b"\n\n\n"):
        text = b"@t\n" + BAD + b"\n+\n" + QUAL + b"\n" + extra
        out, rows = cfr.expected(text, TABLE, K, 2)
        assert out == text.replace(BAD, CLEAN) and len(rows) == 1
    # two substitutions within k of each other: one run that is too long, left alone
    two = b"@t\n" + sub(CLEAN, 10, 13) + b"\n+\n" + QUAL + b"\n"
    out, rows = cfr.expected(two, TABLE, K, 2)
    assert out == two and rows == [(1, 0, 0, 0)]


@pytest.mark.parametrize("text,record,kind", [
    (b">a\nAC\n+\nII\n", 0, "at"),
    (b"@a\nAC\n+\nII\n@b\nAC\n-\nII\n", 1, "plus"),
    (b"@a\nAC\n+\nIII\n", 0, "length"),
    (b"@a\nA C\n+\nIII\n", 0, "blank"),
    (b"@a\nA*C\n+\nIII\n", 0, "blank"),
    (b"@a\nAC\n+\nII\n@b\nAC\n", 1, "incomplete"),
    (b"@a\nAC\n+\nII\n@b\n>C\n+\nII\n", 1, "view"),
    (b"@a\r>b\nAC\n+\nII\n", 0, "view"),
])
def test_rule_refusals(text, record, kind):
    with pytest.raises(cfr.CorrectFastqError) as e:
        cfr.expected(text, TABLE, K, 2)
    assert (e.value.code, e.value.record, e.value.kind) == (cfr.ERR_UNSUPPORTED, record, kind)


def test_rule_argument_and_byte_errors():
    text = b"@a\n" + BAD + b"\n+\n" + QUAL + b"\n"
    for q in (10, 32, 127, 256):
        with pytest.raises(cfr.CorrectFastqError) as e:
            cfr.expected(text, TABLE, K, 2, new_qual=q)
        assert e.value.code == cfr.ERR_ARG
    with pytest.raises(cfr.CorrectFastqError) as e:
        cfr.expected(text, TABLE, K, 0)
    assert e.value.code == cfr.ERR_ARG
    with pytest.raises(cfr.CorrectFastqError) as e:
        cfr.expected(b"@a\nA\xc3C\n+\nIII\n", TABLE, K, 2)
    assert e.value.code == cfr.ERR_NON_ASCII


def test_rule_agrees_with_the_fasta_rule_through_fq2fa():
    """For LF-terminated texts fq2fa of the corrected FASTQ is the corrected FASTA of fq2fa, and the qualities stay."""
    rng = random.Random(7)
    genome = bytes(rng.choice(b"ACGT") for _ in range(400))
    for k in (5, 9):
        table = table_of(genome, k=k, count=3)
        recs = []
        for i in range(24):
            L = rng.choice([0, k - 1, k, k + 1, 2 * k + 3, 4 * k + 9])
            at = rng.randrange(len(genome) - L)
            seq = genome[at:at + L]
            if L and i % 3:
                seq = sub(seq, *rng.sample(range(L), min(L, i % 3)))
            if L > 2 and i % 7 == 0:
                seq = seq[:1] + b"N" + seq[2:]
            recs.append(b"@r%d some words\n" % i + seq + b"\n+" + (b"r%d" % i if i % 2 else b"") + b"\n" +
                        bytes(rng.randrange(33, 127) for _ in range(L)) + b"\n")
        text = b"".join(recs)
        out, rows = cfr.expected(text, table, k, 3)
        fasta, _ = native.fq2fa(text)
        want, want_rows = correct_rule.expected(fasta, table, k, 3)
        # (a read without bases is an empty line behind its header in fq2fa's text and nothing in the FASTA output)
        assert native.fq2fa(out)[0].replace(b"\n\n", b"\n") == want and rows == want_rows and len(out) == len(text)
        assert trim_rule.records(native.fq2fa(out)[0]) == trim_rule.records(want)
        assert sum(r[1] for r in rows) > 0
        before, after = fsr.records(text)[0], fsr.records(out)[0]
        assert [(r[0], r[2], r[3]) for r in before] == [(r[0], r[2], r[3]) for r in after]
        assert cfr.view(text) != text and len(cfr.view(text)) == len(text) and [s for _, s in cfr.parsed(cfr.view(text))] == \
            [fsr.content(r[1]) for r in before]


# ------------------------------------------------------------------------------------------------- layouts
def test_abi_and_struct_layouts():
    assert native.MK_ABI == 6
    rule = native.CorrectFastqRule
    assert C.sizeof(rule) == 16 and [(n, getattr(rule, n).offset, getattr(rule, n).size) for n, _ in rule._fields_] == [
        ("at_least", 0, 8), ("new_qual", 8, 4), ("reserved", 12, 4)]
    st = native.CorrectFastq
    assert st.correct.offset == 0 and st.correct.size == C.sizeof(native.Correct)
    base = C.sizeof(native.Correct)
    assert C.sizeof(native.Correct) == C.sizeof(native.Screen) + 9 * 8 + 6 * 8
    assert [(n, getattr(st, n).offset - base) for n, _ in st._fields_[1:]] == [
        ("lines", 0), ("patched", 8), ("s_copy", 16), ("s_index", 24), ("s_patch", 32)]
    assert C.sizeof(st) == base + 40
    v = st()
    v.lines, v.patched, v.s_patch, v.correct.fixed, v.correct.records = 8, 3, 0.5, 3, 2
    d = v.as_dict()
    assert d["lines"] == 8 and d["patched"] == 3 and d["s_patch"] == 0.5 and d["fixed"] == 3 and d["records"] == 2
    assert {"s_copy", "s_index", "bytes_out", "preamble", "s_gather", "windows"} <= set(d)
    for name in ("mk_correct_fastq_text", "mk_correct_fastq_device"):
        assert name in native.ABI_SYMBOLS and getattr(native.lib(), name).restype is C.c_int


def test_python_layers_are_there():
    sig = inspect.signature(native.Counter.correct_fastq)
    assert list(sig.parameters)[1:] == ["path_or_bytes", "at_least", "new_qual", "fold", "piece_bytes", "info"]
    assert [sig.parameters[n].default for n in ("at_least", "new_qual", "fold", "piece_bytes", "info")] == [2, 0, None, 0, None]
    sig = inspect.signature(native.Counter.correct_fastq_device)
    assert list(sig.parameters)[1:] == ["ptr", "nbytes", "out_ptr", "out_cap", "fix_ptr", "rows_ptr", "cap", "at_least", "new_qual",
                                        "fold"]
    assert [sig.parameters[n].default for n in ("fix_ptr", "rows_ptr", "cap", "at_least", "new_qual", "fold")] == [0, 0, 0, 2, 0, None]
    sig = inspect.signature(kmers.correct_reads_fastq)
    assert list(sig.parameters) == ["table", "file", "out_path", "at_least", "rounds", "tsv_path", "mate_file", "out_path2", "new_qual"]
    assert [sig.parameters[n].default for n in ("at_least", "rounds", "tsv_path", "mate_file", "out_path2", "new_qual")] == [
        2, 1, None, None, None, 0]
    # correct_reads keeps the arguments it has
    assert list(inspect.signature(kmers.correct_reads).parameters) == ["table", "file", "out_path", "at_least", "rounds", "tsv_path",
                                                                       "mate_file", "out_path2"]
    assert native.quality_byte("I") == 73 and native.quality_byte(b"!") == 33 and native.quality_byte(0) == 0 and \
        native.quality_byte(40) == 40
    with pytest.raises(ValueError):
        native.quality_byte("II")


# ------------------------------------------------------------------------------------------- kmers and CLI
@pytest.fixture()
def files(tmp_path):
    (tmp_path / "s.fna").write_bytes(b">s\nACGTACGTAC\n")
    (tmp_path / "r.fastq").write_bytes(b"@a\nACGTA\n+\nIIIII\n")
    (tmp_path / "r2.fq").write_bytes(b"@a\nACGTA\n+\nIIIII\n")
    (tmp_path / "r.fna").write_bytes(b">a\nACGT\n")
    return tmp_path


def test_kmers_value_errors(files):
    """Refused before the table is touched (None stands for it here)."""
    out = files / "o.fastq"
    with pytest.raises(ValueError, match="FASTQ"):
        kmers.correct_reads_fastq(None, files / "r.fna", out)
    with pytest.raises(ValueError, match="FASTQ"):  # (the mate too)
        kmers.correct_reads_fastq(None, files / "r.fastq", out, mate_file=files / "r.fna", out_path2=files / "o2.fastq")
    with pytest.raises(ValueError, match="rounds"):
        kmers.correct_reads_fastq(None, files / "r.fastq", out, rounds=0)
    with pytest.raises(ValueError, match="out_path2"):
        kmers.correct_reads_fastq(None, files / "r.fastq", out, out_path2=files / "o2.fastq")
    with pytest.raises(ValueError, match="new_qual"):
        kmers.correct_reads_fastq(None, files / "r.fastq", out, new_qual=" ")
    with pytest.raises(ValueError, match="new_qual"):
        kmers.correct_reads_fastq(None, files / "r.fastq", out, new_qual="II")
    assert not out.exists()


def parse(files, *extra):
    return cli.parseargs(["-i", str(files / "s.fna"), "-k", "5", "-skipclean", "-o", str(files / "out")] + [str(x) for x in extra])[0]


def test_cli_accepts(files):
    args = parse(files, "-correct", files / "r.fastq", "-correct_fastq", "-correct_qual", "!")
    assert args.correct_fastq and args.correct_qual == "!"
    args = parse(files, "-correct", files / "r.fastq", "-correct_mate", files / "r2.fq", "-correct_fastq")
    assert args.correct_fastq and args.correct_qual is None
    args = parse(files, "-correct", files / "r.fastq")
    assert not args.correct_fastq


@pytest.mark.parametrize("extra,message", [
    (("-correct_fastq",), "-correct_fastq needs -correct FILE"),
    (("-correct_qual", "I"), "-correct_qual needs -correct FILE"),
    (("-correct", "r.fna", "-correct_fastq"), "not a FASTQ file"),
    (("-correct", "r.fastq", "-correct_qual", "I"), "-correct_qual needs -correct_fastq"),
    (("-correct", "r.fastq", "-correct_fastq", "-correct_qual", "II"), "one printable character"),
    (("-correct", "r.fastq", "-correct_fastq", "-correct_qual", " "), "one printable character"),
    (("-correct", "r.fastq", "-correct_fastq", "-correct_qual", "\x7f"), "one printable character"),
    (("-trim", "r.fastq", "-correct", "r.fastq", "-fastq_out"), "does not go with -correct"),
])
def test_cli_refuses(files, capsys, extra, message):
    argv = [str(files / x) if x.startswith("r.") else x for x in extra]
    with pytest.raises(SystemExit) as e:
        parse(files, *argv)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_cli_refuses_a_fasta_mate(files, capsys):
    (files / "m.fna").write_bytes(b">a\nACGT\n")
    with pytest.raises(SystemExit) as e:  # (a FASTA mate is a nucleotide file like the FASTQ one: only this flag objects)
        parse(files, "-correct", files / "r.fastq", "-correct_mate", files / "m.fna", "-correct_fastq")
    assert e.value.code == 2 and "not a FASTQ file" in capsys.readouterr().err
