"""Host side of reading count tables back (mk_tsv_shape, the -tsv flag): no GPU is touched.  What a table looks like is
restated here in plain Python from the line rules of include/mercat_hip.h and compared with the native helper on every
count table the repository keeps."""
import re
from pathlib import Path

import pytest

from mercat2_amd import cli, native

GOLDEN = Path(__file__).parent / "golden"
TABLES = sorted((GOLDEN / "tsv").glob("*.tsv")) + sorted((GOLDEN / "report").glob("in_*.tsv"))


def _is_row(line: bytes) -> bool:
    """k key bytes (k >= 1, up to the LAST tab: a key may hold tabs, a count cannot), a tab, 1-20 digits < 2^64."""
    key, tab, count = line.rpartition(b"\t")
    return bool(tab) and len(key) >= 1 and re.fullmatch(rb"[0-9]{1,20}", count) is not None and int(count) < 1 << 64


def _shape(path: Path) -> dict:
    lines = path.read_bytes().split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    header = bool(lines) and not _is_row(lines[0])
    column = ""
    if header:
        fields = lines[0].split(b"\t")
        column = fields[1].decode() if len(fields) > 1 else ""
    rows = lines[1 if header else 0:][:4096]
    keys = [r.rpartition(b"\t")[0] for r in rows]
    if not keys:
        alphabet = native.ALPHABET_RAW
    elif all(set(k) <= set(b"ACGT") for k in keys):
        alphabet = native.ALPHABET_NT2
    elif all(set(k) <= set(range(ord("A"), ord("Z") + 1)) for k in keys):
        alphabet = native.ALPHABET_AA5
    else:
        alphabet = native.ALPHABET_RAW
    return {"k": len(keys[0]) if keys else 0, "header": header, "column": column, "alphabet": alphabet}


def test_there_are_tables_to_look_at():
    assert len(TABLES) >= 15


@pytest.mark.parametrize("path", TABLES, ids=lambda p: p.name)
def test_shape_of_committed_tables(path):
    got = native.tsv_shape(path)
    assert got == _shape(path)
    assert got["header"] and got["column"].endswith("_Count")
    m = re.search(r"_k(\d+)_c", path.name)
    if m:  # (tests/golden/tsv names its files <input>_k<k>_c<min_count>)
        assert got["k"] == int(m.group(1))
    else:
        assert got["k"] == 5  # tests/golden/report/in_*.tsv


def test_shape_names_the_alphabets():
    hint = {p.name: native.tsv_shape(p)["alphabet"] for p in TABLES}
    assert hint["A_k31_c1.tsv"] == native.ALPHABET_NT2
    assert hint["ref_DJ_pro_k5_c10_s1.tsv"] == native.ALPHABET_AA5
    assert hint["Scaffolds_with-NNN_k5_c10.tsv"] == native.ALPHABET_RAW  # (keys with N and lower case: kept as text)


def test_shape_of_a_headerless_table(tmp_path):
    """What Jellyfish and KMC dump: 'kmer\\tcount' rows from the first line on."""
    p = tmp_path / "dump.tsv"
    p.write_bytes(b"ACGTA\t7\nCCCCC\t18446744073709551615\nGGGTA\t1")
    assert native.tsv_shape(p) == {"k": 5, "header": False, "column": "", "alphabet": native.ALPHABET_NT2} == _shape(p)
    p.write_bytes(b"MKVLA\t3\nACGTA\t2\n")
    assert native.tsv_shape(p) == {"k": 5, "header": False, "column": "", "alphabet": native.ALPHABET_AA5}
    p.write_bytes(b"ACGTA\t18446744073709551616\nCCCCC\t1\n")  # (line 1 is no data row: its count does not fit)
    assert native.tsv_shape(p) == {"k": 5, "header": True, "column": "18446744073709551616", "alphabet": native.ALPHABET_NT2}


def test_shape_of_tables_without_rows(tmp_path):
    p = tmp_path / "empty.tsv"
    p.write_bytes(b"")
    assert native.tsv_shape(p) == {"k": 0, "header": False, "column": "", "alphabet": native.ALPHABET_RAW}
    p.write_bytes(b"k-mer\tX_Count\n")
    assert native.tsv_shape(p) == {"k": 0, "header": True, "column": "X_Count", "alphabet": native.ALPHABET_RAW}
    with pytest.raises(native.MercatHipError) as e:
        native.tsv_shape(tmp_path / "missing.tsv")
    assert e.value.code == -6


def test_binding_knows_the_loader():
    assert native.MK_ABI == 6
    for name in ("mk_load_tsv", "mk_load_tsv_text", "mk_tsv_shape"):
        assert name in native.ABI_SYMBOLS and getattr(native.lib(), name) is not None
    assert [n for n, _ in native.TsvLoad._fields_] == ["bytes", "lines", "rows", "packed_rows", "text_rows", "zero_rows",
                                                        "new_rows", "header", "pieces", "s_read", "s_parse", "s_import", "s_total"]
    import ctypes
    assert ctypes.sizeof(native.TsvLoad) == 7 * 8 + 2 * 4 + 4 * 8


def _result_folder(tmp_path, k=5):
    out = tmp_path / "old"
    (out / "tsv_nucleotide").mkdir(parents=True)
    (out / "tsv_protein").mkdir()
    (out / "tsv_nucleotide" / "s1_counts.tsv").write_bytes(b"k-mer\ts1_Count\n" + b"A" * k + b"\t12\n")
    (out / "tsv_protein" / "p1_counts.tsv").write_bytes(b"k-mer\tp1_Count\n" + b"M" * k + b"\t11\n")
    (out / "tsv_protein" / "notes.txt").write_text("not a table")
    return out


def test_parseargs_accepts_tsv_alone(tmp_path):
    out = _result_folder(tmp_path)
    args, _ = cli.parseargs(["-tsv", str(out), "-k", "5"])
    assert args.i == [] and args.f is None
    assert {kind: sorted(v) for kind, v in args.loaded.items()} == {"nucleotide": ["s1"], "protein": ["p1"]}
    assert args.loaded["protein"]["p1"] == out / "tsv_protein" / "p1_counts.tsv"
    # a tsv_<type> folder itself
    args, _ = cli.parseargs(["-tsv", str(out / "tsv_protein"), "-k", "5"])
    assert {kind: sorted(v) for kind, v in args.loaded.items()} == {"nucleotide": [], "protein": ["p1"]}
    # beside -i
    args, _ = cli.parseargs(["-tsv", str(out), "-i", str(GOLDEN / "inputs" / "A.fasta"), "-k", "5"])
    assert args.i and sorted(args.loaded["nucleotide"]) == ["s1"]


def test_parseargs_still_wants_an_input(capsys):
    with pytest.raises(SystemExit) as e:
        cli.parseargs(["-k", "5"])
    assert e.value.code == 2
    assert "Please provide either an input file (-i) or an input folder (-f)" in capsys.readouterr().err


def test_parseargs_refuses_another_k_and_a_missing_folder(tmp_path, capsys):
    out = _result_folder(tmp_path)
    with pytest.raises(SystemExit) as e:
        cli.parseargs(["-tsv", str(out), "-k", "6"])
    assert e.value.code == 2 and "holds 5-mers" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        cli.parseargs(["-tsv", str(tmp_path / "nowhere"), "-k", "5"])
    assert e.value.code == 2


def test_the_slow_reader_is_gone():
    from mercat2_amd import diversity, harness, report
    assert not hasattr(report, "_load_tsv") and not hasattr(diversity, "_load_tsv")
    assert callable(harness.load_table) and callable(native.counter_from_tsv) and callable(native.Counter.load_tsv)
