"""Paired reads on the host: mk_interleave / mk_split_pairs (native.interleave, native.split_pairs), the CLI's paired
flags and the paired columns of the per-record TSVs.  No GPU.  The record rule is restated here in plain Python: a record
starts at the first byte of a line whose first non-blank byte is '>', lines end at LF, CR LF or a lone CR."""
import ctypes
import re

import numpy as np
import pytest

from mercat2_amd import cli, native, report

RANGE, ARG = -7, -1
_LINE = re.compile(rb"[^\r\n]*(?:\r\n|\r|\n)|[^\r\n]+")
_BLANKS = b" \t\x0b\x0c\x1c\x1d\x1e\x1f"


def records(text: bytes):
    """(preamble, [raw bytes of every record]) by the filter's rule."""
    pre, recs = b"", []
    for line in _LINE.findall(text):
        if line.lstrip(_BLANKS).startswith(b">"):
            recs.append(line)
        elif recs:
            recs[-1] += line
        else:
            pre += line
    return pre, recs


def closed(rec: bytes) -> bytes:
    return rec if rec[-1:] in (b"\n", b"\r") else rec + b"\n"


TEXTS = {
    "lf": (b">a 1\nACGT\n>b\nGG\nTT\n>c\n", b">a 2\nTTTT\n>b\nC\n>c\nAAAA\n"),
    "crlf": (b">a 1\r\nACGT\r\n>b\r\nGG\r\nTT\r\n", b">a 2\r\nTTTT\r\n>b\r\nC\r\n"),
    "lone_cr": (b">a 1\rACGT\r>b\rGG\rTT\r", b">a 2\rTTTT\r>b\rC\r"),
    "mixed_ends": (b">a\r\nAC\rGT\n>b\nGG\r", b">a\nTT\r\n>b\rC\n"),
    "wrapped": (b">a\nACGT\nACGT\nAC\n>b\nGG\n", b">a\nT\nT\nT\n>b\nCCCC\nCC\n"),
    "leading_blanks": (b"  >a\nACGT\n\t >b\nGG\n", b" \x0b>a\nTT\n>b\nC\n"),
    "preamble": (b"\n  \n\t\n>a\nACGT\n>b\nGG\n", b"**\n\n>a\nTT\n>b\nC\n"),
    "no_final_newline": (b">a\nACGT\n>b\nGG", b">a\nTT\n>b\nC"),
    "empty_records": (b">a\n>b\n\n>c\nAC\n>d", b">a\nTT\n>b\n>c\n>d\n"),
    "gt_inside": (b">a x>y\nAC>GT\n>b\nGG\n", b">a\nT >\n>b\nC\n"),
    "long": (b"".join(b">r%d\n%s\n" % (i, b"ACGT" * (i % 40)) for i in range(300)),
             b"".join(b">r%d\r\n%s\r\n" % (i, b"TTGA" * (i % 23)) for i in range(300))),
}


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_interleave_then_split_is_the_identity(name):
    a, b = TEXTS[name]
    (_, ra), (_, rb) = records(a), records(b)
    assert len(ra) == len(rb) > 0
    both = native.interleave(a, b)
    assert both == b"".join(closed(x) + closed(y) for x, y in zip(ra, rb))
    assert records(both) == (b"", [closed(r) for pair in zip(ra, rb) for r in pair])  # (a record stays a record)
    one, two = native.split_pairs(both)
    assert one == b"".join(closed(r) for r in ra) and two == b"".join(closed(r) for r in rb)
    # the texts minus their preambles, and the newline a last record gains
    assert one == closed(a[len(records(a)[0]):]) and two == closed(b[len(records(b)[0]):])
    assert native.interleave(one, two) == both


def test_split_takes_records_byte_for_byte():
    text = b">a\nAC\n  >b\r\nGG\r\n>c\rTT\r>d\nC"  # (the last record keeps its missing newline)
    one, two = native.split_pairs(text)
    assert one == b">a\nAC\n>c\rTT\r" and two == b"  >b\r\nGG\r\n>d\nC"
    assert native.split_pairs(b"ACGT\n>b\nGG\n") == (b"ACGT\n", b">b\nGG\n")  # the headless record is a first mate


def test_unequal_counts_and_odd_counts_are_range_errors():
    with pytest.raises(native.MercatHipError) as e:
        native.interleave(b">a\nAC\n>b\nGG\n>c\nT\n", b">a\nTT\n")
    assert e.value.code == RANGE and "3 records" in str(e.value) and "1" in str(e.value)
    with pytest.raises(native.MercatHipError) as e:
        native.split_pairs(b">a\nAC\n>b\nGG\n>c\nT\n")
    assert e.value.code == RANGE and "3 records" in str(e.value)
    with pytest.raises(native.MercatHipError) as e:  # sequence in front of the first header line cannot be interleaved
        native.interleave(b">a\nAC\n", b"GG\n>a\nTT\n")
    assert e.value.code == ARG and "text2" in str(e.value)


def test_zero_records():
    assert native.interleave(b"", b"") == b"" and native.interleave(b"\n \n", b"") == b""
    assert native.split_pairs(b"") == (b"", b"") and native.split_pairs(b"\n\n") == (b"", b"")


def test_capacities():
    L = native.lib()
    a, b = TEXTS["no_final_newline"]
    want = native.interleave(a, b)
    ka, kb = np.frombuffer(a, dtype=np.uint8), np.frombuffer(b, dtype=np.uint8)
    n, pairs = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.mk_interleave(ka.ctypes.data, len(a), kb.ctypes.data, len(b), None, 0, ctypes.byref(n), ctypes.byref(pairs)) == RANGE
    assert n.value == len(want) == len(a) + len(b) + 2 and pairs.value == 2
    out = np.full(len(want) + 1, 0xA5, dtype=np.uint8)
    assert L.mk_interleave(ka.ctypes.data, len(a), kb.ctypes.data, len(b), out.ctypes.data, len(want) - 1, ctypes.byref(n), None) == RANGE
    assert out[len(want) - 1:].tolist() == [0xA5, 0xA5]  # nothing past the room it was told
    assert L.mk_interleave(ka.ctypes.data, len(a), kb.ctypes.data, len(b), out.ctypes.data, len(want), ctypes.byref(n), None) == 0
    assert out[:-1].tobytes() == want and out[-1] == 0xA5


def test_abi_and_symbols():
    assert native.MK_ABI == 6
    L = native.lib()
    for name in ("mk_pairs_text", "mk_pairs_device", "mk_interleave", "mk_split_pairs", "mk_host_error"):
        assert name in native.ABI_SYMBOLS and hasattr(L, name)
    assert ctypes.sizeof(native.PairsRule) == 8 + 24 + 16 + 24
    assert ctypes.sizeof(native.Pairs) == ctypes.sizeof(native.Screen) + 15 * 8 + 5 * 8
    assert (native.PAIRS_FOLD, native.PAIRS_INVERT, native.PAIRS_BOTH) == (1, 2, 4)


def test_paired_tsv_columns():
    names, lengths, kept = ["a/1", "a/2", "b/1", "b/2"], [50, 50, 40, 40], [50, 31, 0, 40]
    assert report.format_trim_tsv(names, lengths, kept) == b"record\tlength\tkept\na/1\t50\t50\na/2\t50\t31\nb/1\t40\t0\nb/2\t40\t40\n"
    assert report.format_trim_tsv(names, lengths, kept, [1, 1, 0, 2]) == (
        b"record\tlength\tkept\temitted\tpair\na/1\t50\t50\tpair\t0\na/2\t50\t31\tpair\t0\nb/1\t40\t0\t0\t1\nb/2\t40\t40\tsingle\t1\n")
    assert report.format_norm_tsv(names, [20, 20, 10, 10], [5, 7, 0, 9], [1, 1, 0, 0]).startswith(b"record\twindows\tmedian\tkept\n")
    assert report.format_norm_tsv(names, [20, 20, 10, 10], [5, 7, 0, 9], [1, 1, 0, 0], paired=True) == (
        b"record\twindows\tmedian\tkept\tpair\na/1\t20\t5\t1\t0\na/2\t20\t7\t1\t0\nb/1\t10\t0\t0\t1\nb/2\t10\t9\t0\t1\n")


# ------------------------------------------------------------------------------------------------------ the CLI
@pytest.fixture()
def files(tmp_path):
    for name in ("s.fna", "r1.fa", "r2.fa", "p.faa"):
        (tmp_path / name).write_bytes(b">a\nACGTACGTAC\n")
    return tmp_path


def parse(files, *extra):
    return cli.parseargs(["-i", str(files / "s.fna"), "-k", "5", "-skipclean", "-o", str(files / "out")] + [str(x) for x in extra])[0]


def test_cli_accepts_the_paired_flags(files):
    args = parse(files, "-trim", files / "r1.fa", "-paired", "-singles")
    assert args.pairs_of == {"filter": False, "trim": True, "norm": False} and args.singles
    assert cli.paired_outputs(args, "trim", files, "s_trimmed", "s", "fna") == {
        "out_path": files / "s_trimmed.fna", "paired": True, "mate_file": None, "out_path2": None, "singles_path": files / "s_singles.fna"}
    args = parse(files, "-filter", files / "r1.fa", "-filter_mate", files / "r2.fa", "-filter_pair", "both", "-filter_keep", "matched")
    assert args.pairs_of["filter"] and args.filter_pair == "both"
    where = cli.paired_outputs(args, "filter", files, "s_matched", "s", "fna")
    assert where["out_path"] == files / "s_matched_1.fna" and where["out_path2"] == files / "s_matched_2.fna"
    assert where["mate_file"] == str(files / "r2.fa") and "singles_path" not in where
    args = parse(files, "-norm", files / "r1.fa")
    assert not any(args.pairs_of.values()) and args.filter_pair == "either"
    assert cli.paired_outputs(args, "norm", files, "s_kept", "s", "fna") == {"out_path": files / "s_kept.fna"}


@pytest.mark.parametrize("extra,message", [
    (("-paired",), "-paired needs"),
    (("-trim_mate", "r2.fa"), "-trim_mate needs -trim"),
    (("-filter_mate", "r2.fa", "-trim", "r1.fa"), "-filter_mate needs -filter"),
    (("-norm", "r1.fa", "-norm_mate", "r2.fa", "-paired"), "does not go with -norm_mate"),
    (("-trim", "r1.fa", "-trim_mate", "missing.fa"), "is not valid"),
    (("-trim", "r1.fa", "-trim_mate", "p.faa"), "not the type of -trim"),
    (("-filter", "r1.fa", "-filter_pair", "both"), "-filter_pair needs"),
    (("-trim", "r1.fa", "-paired", "-filter_pair", "both"), "-filter_pair needs"),
    (("-trim", "r1.fa", "-singles"), "-singles needs"),
    (("-filter", "r1.fa", "-paired", "-singles"), "-filter_keep matched"),
    (("-norm", "r1.fa", "-paired", "-singles", "-norm_keep", "tossed"), "-norm_keep kept"),
    (("-filter", "r1.fa", "-paired", "-filter_pair", "neither"), "invalid choice"),
])
def test_cli_refuses(files, capsys, extra, message):
    argv = [str(files / x) if x.endswith((".fa", ".faa")) else x for x in extra]
    with pytest.raises(SystemExit) as e:
        parse(files, *argv)
    assert e.value.code == 2 and message in capsys.readouterr().err
