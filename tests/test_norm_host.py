"""Host-side checks of the normalisation calls (mk_norm_text / mk_norm_device): the rule's plain-Python restatement
(tests/norm_rule.py) against hand examples and the statistics of its hash, header, binding, report format and CLI layers.
No kernel is launched here; tests/test_gpu_norm.py normalises on the GPU."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import norm_rule
from conftest import GOLDEN, ROOT
from mercat2_amd import cli, kmers, native, report
from test_trim_host import CTYPE, HEADER, _layout, _struct_fields

HAND_TABLE = {"ACG": 2, "CGT": 9, "GTA": 1, "TAC": 5_000_000_000}


# ------------------------------------------------------------------------------------------------ the rule
def test_the_hash_keeps_a_quarter():
    """2000 records of median 4 x target: each is kept with probability 1 / 4, so 500 +- 97 (5 sigma of Binomial(2000,
    1 / 4): sqrt(2000 * 3 / 16) = 19.4) are -- under any seed, and different ones under different seeds."""
    kept = {seed: [norm_rule.kept_of(10, 80, r, 20, seed=seed) for r in range(2000)] for seed in (0, 1, 2 ** 63)}
    for flags in kept.values():
        assert abs(sum(flags) - 500) <= 97
    assert kept[0] != kept[1] != kept[2 ** 63]
    assert norm_rule.u_of(0, 0) == 0xE220A8397B1DCDAF >> 32  # splitmix64's first output from state 0


def test_rule_details():
    k = 3
    # medians: ACGTAC -> counts [2, 9, 1, 5e9 clipped] sorted [1, 2, 9, 2^32 - 1], element 2 = 9
    text = b"\n \nACGT\n>r x\nACG*TAC\n  >b\rAC\rG\r>h\n>e\n\n>last\nTACTAC"
    res = norm_rule.expected(text, HAND_TABLE, k, 5)
    assert res["median"] == [9, 9, 2, 0, 0, 2 ** 32 - 1] and res["windows"] == [2, 4, 1, 0, 0, 4]
    assert res["records_short"] == 2 and res["records_over"] == 3 and res["records_low"] == 0
    assert res["keep"][2] and not res["keep"][3] and not res["keep"][4]
    inv = norm_rule.expected(text, HAND_TABLE, k, 5, invert=True)
    assert [a != b for a, b in zip(res["keep"], inv["keep"])] == [True] * 6
    assert sorted(res["out"] + inv["out"]) == sorted(text) and norm_rule.preamble(text) == 0
    assert res["records_out"] + inv["records_out"] == 6 and res["records_thinned"] == 3 - sum(res["keep"][i] for i in (0, 1, 5))
    # at min_depth and below it; at target and above it
    assert norm_rule.expected(text, HAND_TABLE, k, 9, min_depth=9)["keep"] == [True, True, False, False, False, norm_rule.kept_of(4, 2 ** 32 - 1, 5, 9)]
    assert norm_rule.expected(text, HAND_TABLE, k, 9, min_depth=3)["records_low"] == 1
    assert norm_rule.expected(text, HAND_TABLE, k, 2 ** 32 - 1)["keep"] == [True, True, True, False, False, True]
    assert norm_rule.preamble(b" \n\n>a\nACG") == 3 and norm_rule.expected(b" \n\n>a\nACG", HAND_TABLE, k, 5)["out"] == b">a\nACG"
    assert norm_rule.median_of([]) == 0 and norm_rule.median_of([7]) == 7 and norm_rule.median_of([3, 1]) == 3


# ---------------------------------------------------------------------------------------------- the header
def test_header_declares_the_calls_and_flags():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ("mk_norm_text", "mk_norm_device"):
        assert re.search(r"\bint %s\s*\(mk_ctx\*" % name, code)
        assert name in native.ABI_SYMBOLS and getattr(native.lib(), name) is not None
    assert re.search(r"#define MK_NORM_FOLD\s+1u", code) and re.search(r"#define MK_NORM_INVERT\s+2u", code)
    assert (native.NORM_FOLD, native.NORM_INVERT) == (1, 2)
    select_min = int(re.search(r"#define MK_MEDIAN_SELECT_MIN\s+(\d+)u", code).group(1))
    assert native.MEDIAN_SELECT_MIN == select_min and 8192 <= select_min <= 1 << 22
    args = re.search(r"int mk_norm_text\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "ctx", "text", "n", "piece_bytes", "flags", "rule", "out", "out_cap", "out_len", "median", "keep", "rows", "cap", "nrows", "st"]
    args = re.search(r"int mk_norm_device\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "ctx", "d_text", "n", "flags", "rule", "d_out", "out_cap", "out_len", "d_median", "d_keep", "d_rows", "cap", "nrows", "st"]
    assert len(native.lib().mk_norm_text.argtypes) == 15 and len(native.lib().mk_norm_device.argtypes) == 14
    assert code.index("mk_trim_device") < code.index("MK_NORM_FOLD") < code.index("mk_norm_rule_t") < code.index("mk_norm_text") \
        < code.index("mk_norm_device") < code.index("mk_merged_export")
    assert "streaming" in HEADER and "order" in HEADER  # why khmer's streaming form is not this


def test_bound_structs_match_the_header():
    want_size, _, want = _layout("mk_norm_t")
    assert [f for f, _ in want] == [g[0] for g in native.Norm._fields_]
    assert [(f, getattr(native.Norm, f).offset) for f, _ in want] == want
    assert C.sizeof(native.Norm) == want_size == 96 + 7 * 8 + 5 * 8 == 192
    for (ctype, field), (_, got) in zip(_struct_fields("mk_norm_t"), native.Norm._fields_):
        assert got is (native.Screen if ctype == "mk_screen_t" else CTYPE[ctype]), field
    assert [f for _, f in _struct_fields("mk_norm_t")[1:]] == [
        "records_out", "records_short", "records_low", "records_over", "records_thinned", "bytes_out", "preamble",
        "s_place", "s_track", "s_median", "s_gather", "s_write"]
    want_size, _, want = _layout("mk_norm_rule_t")
    assert want == [("target", 0), ("min_depth", 8), ("seed", 16)] and C.sizeof(native.NormRule) == want_size == 24
    assert [(f, getattr(native.NormRule, f).offset) for f, _ in native.NormRule._fields_] == want
    st = native.Norm()
    st.screen.records, st.records_out, st.records_thinned, st.s_median = 7, 5, 2, 0.5
    d = st.as_dict()
    assert d["records"] == 7 and d["records_out"] == 5 and d["records_thinned"] == 2 and d["s_median"] == 0.5
    assert {"records_short", "records_low", "records_over", "bytes_out", "preamble", "s_place", "s_track", "s_gather", "s_write"} <= set(d)


def test_the_abi_number_stands():
    assert native.MK_ABI == 6 and native.lib().mk_version().decode().split()[1].split(".")[0] == "6"


def test_python_layers_are_there():
    for name in ("normalize", "normalize_device"):
        assert callable(getattr(native.Counter, name))
    assert list(inspect.signature(native.Counter.normalize).parameters)[1:] == [
        "path_or_bytes", "target", "min_depth", "seed", "invert", "fold", "piece_bytes", "info"]
    sig = inspect.signature(kmers.normalize_reads).parameters
    assert list(sig) == ["table", "file", "out_path", "target", "min_depth", "seed", "invert", "tsv_path"] and sig["target"].default == 20
    assert "FASTQ" in kmers.normalize_reads.__doc__ and "fq2fa" in kmers.normalize_reads.__doc__
    assert callable(report.write_norm_tsv)


# ----------------------------------------------------------------------------------------------- the report
def test_norm_tsv_format(tmp_path):
    names = ["r1", "", "gone"]
    windows = np.array([120, 18446744073709551615, 0], dtype=np.uint64)
    median = np.array([97, 4294967295, 0], dtype=np.uint32)
    kept = np.array([True, False, False])
    want = b"record\twindows\tmedian\tkept\nr1\t120\t97\t1\n\t18446744073709551615\t4294967295\t0\ngone\t0\t0\t0\n"
    assert report.write_norm_tsv(tmp_path / "t.tsv", names, windows, median, kept) == 3 and (tmp_path / "t.tsv").read_bytes() == want
    assert report.format_norm_tsv([], windows[:0], median[:0], kept[:0]) == b"record\twindows\tmedian\tkept\n"
    with pytest.raises(ValueError):
        report.write_norm_tsv(tmp_path / "x.tsv", names, windows, median, kept[:2])


# -------------------------------------------------------------------------------------------------- the CLI
def test_cli_accepts(tmp_path):
    fasta = str(GOLDEN / "inputs" / "A.fasta")
    args, _ = cli.parseargs(["-i", fasta, "-k", "5", "-norm", fasta])
    assert (args.norm, args.norm_kind, args.norm_target, args.norm_min, args.norm_seed, args.norm_keep) == (fasta, "nucleotide", 20, 0, 0, "kept")
    args, _ = cli.parseargs(["-i", fasta, "-k", "5", "-norm", fasta, "-norm_target", "4294967295", "-norm_min", "3", "-norm_seed",
                             str(2 ** 64 - 1), "-norm_keep", "tossed"])
    assert (args.norm_target, args.norm_min, args.norm_seed, args.norm_keep) == (2 ** 32 - 1, 3, 2 ** 64 - 1, "tossed")
    for name, kind in (("x.faa.gz", "protein"), ("x.fastq.gz", "nucleotide"), ("x.fq", "nucleotide"), ("x.fna", "nucleotide")):
        (tmp_path / name).write_bytes(b"")
        assert cli.parseargs(["-i", fasta, "-k", "5", "-norm", str(tmp_path / name)])[0].norm_kind == kind
    args, _ = cli.parseargs(["-i", fasta, "-k", "5"])
    assert args.norm is None and args.norm_kind is None and args.norm_target is None and args.norm_keep is None


def test_cli_rejects(tmp_path, capsys):
    fasta = str(GOLDEN / "inputs" / "A.fasta")
    out = tmp_path / "out"
    for extra in (["-norm", str(tmp_path / "missing.fa")], ["-norm", str(ROOT / "README.md")], ["-norm_target", "20"], ["-norm_min", "1"],
                  ["-norm_seed", "1"], ["-norm_keep", "kept"], ["-norm", fasta, "-norm_target", "0"], ["-norm", fasta, "-norm_target", "-1"],
                  ["-norm", fasta, "-norm_target", str(2 ** 32)], ["-norm", fasta, "-norm_min", "-1"],
                  ["-norm", fasta, "-norm_min", str(2 ** 32)], ["-norm", fasta, "-norm_seed", "-1"],
                  ["-norm", fasta, "-norm_seed", str(2 ** 64)], ["-norm", fasta, "-norm_keep", "both"], ["-norm", fasta, "-norm_target", "x"]):
        with pytest.raises(SystemExit) as e:
            cli.main(["-i", fasta, "-k", "5", "-o", str(out)] + extra)
        assert e.value.code == 2 and not out.exists(), extra  # (before the output folder is made, before any counting)
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        cli.parseargs(["-h"])
    text = " ".join(capsys.readouterr().out.split())
    assert e.value.code == 0 and "-norm FILE" in text and "-norm_target" in text and "-norm_min" in text and "-norm_seed" in text
    assert "-norm_keep" in text and "_norm.tsv" in text
