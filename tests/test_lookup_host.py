"""Host side of the k-mer lookup (mk_lookup*, Counter.lookup*, report.write_query_tsv, the -query flag): the binding, the
ABI number, the argument parser and the query table's formatter.  No GPU is touched."""
import ctypes
import re
from pathlib import Path

import pytest

from mercat2_amd import cli, native, report

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).parent / "golden"
SYMBOLS = ("mk_lookup", "mk_lookup_device", "mk_lookup_text", "mk_lookup_file")


def test_header_binding_and_library_agree_on_the_lookup():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mercat_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(mk_[a-z0-9_]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared and name in native.ABI_SYMBOLS and getattr(native.lib(), name) is not None
    assert re.search(r"#define\s+MK_LOOKUP_FOLD\s+1u", header) and native.LOOKUP_FOLD == 1


def test_lookup_struct_layout(tmp_path):
    assert ctypes.sizeof(native.Lookup) == 88 == 7 * 8 + 2 * 4 + 3 * 8
    assert [n for n, _ in native.Lookup._fields_] == ["bytes", "lines", "keys", "found", "packed_keys", "text_keys", "folded",
                                                       "header", "pieces", "s_read", "s_probe", "s_total"]
    import subprocess
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mercat_hip.h"\n'
                   'int main(){printf("%zu %zu %zu",sizeof(mk_lookup_t),offsetof(mk_lookup_t,header),offsetof(mk_lookup_t,s_read));return 0;}\n')
    subprocess.check_call(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(tmp_path / "sz")])
    assert subprocess.check_output([str(tmp_path / "sz")]).decode().split() == [
        "88", str(native.Lookup.header.offset), str(native.Lookup.s_read.offset)]


def test_abi_number_stays_and_the_minor_moves():
    assert native.MK_ABI == 6
    assert native.lib().mk_version().decode().startswith("mercat_hip 6.1")


def _result_folder(tmp_path, k=5):
    out = tmp_path / "old"
    (out / "tsv_nucleotide").mkdir(parents=True)
    (out / "tsv_nucleotide" / "s1_counts.tsv").write_bytes(b"k-mer\ts1_Count\n" + b"A" * k + b"\t12\n")
    return out


def test_parseargs_accepts_query(tmp_path, capsys):
    out = _result_folder(tmp_path)
    panel = tmp_path / "panel.txt"
    panel.write_bytes(b"AAAAA\nACGTA\n")
    args, _ = cli.parseargs(["-tsv", str(out), "-k", "5", "-query", str(panel)])
    assert args.query == str(panel) and args.i == [] and sorted(args.loaded["nucleotide"]) == ["s1"]
    args, _ = cli.parseargs(["-i", str(GOLDEN / "inputs" / "A.fasta"), "-k", "5", "-query", str(panel)])
    assert args.query == str(panel) and args.i
    args, _ = cli.parseargs(["-i", str(GOLDEN / "inputs" / "A.fasta"), "-k", "5"])
    assert args.query is None
    with pytest.raises(SystemExit) as e:
        cli.parseargs(["-tsv", str(out), "-k", "5", "-query", str(tmp_path / "missing.txt")])
    assert e.value.code == 2 and "is not valid" in capsys.readouterr().err


def test_query_table_bytes():
    """Panel order, a duplicate kept, a key that holds a tab, names as given (the caller sorts them)."""
    keys = [b"ACGTA", b"A\tG A", b"ACGTA", b"NNNNN"]
    got = report.format_query_tsv(["a", "b"], keys, [[3, 0, 3, 18446744073709551615], [0, 7, 0, 0]])
    assert got == (b"k-mer\ta\tb\n"
                   b"ACGTA\t3\t0\n"
                   b"A\tG A\t0\t7\n"
                   b"ACGTA\t3\t0\n"
                   b"NNNNN\t18446744073709551615\t0\n")
    assert report.format_query_tsv(["only"], [], [[]]) == b"k-mer\tonly\n"


def test_panel_keys_follow_the_row_rules(tmp_path):
    p = tmp_path / "panel.tsv"
    p.write_bytes(b"k-mer\tx_Count\nACGTA\t12\nA\tG A\nTTTTT")
    assert report.panel_keys(p, 5, True) == [b"ACGTA", b"A\tG A", b"TTTTT"]
    p.write_bytes(b"ACGTA\nCCCCC\t1\n")
    assert report.panel_keys(p, 5, False) == [b"ACGTA", b"CCCCC"]


def test_python_layers_are_there():
    from mercat2_amd import kmers
    for name in ("lookup", "lookup_text", "lookup_device"):
        assert callable(getattr(native.Counter, name))
    assert callable(native.lookup_multi) and callable(kmers.lookup_kmers) and callable(report.write_query_tsv)


def test_no_new_environment_switch():
    text = (ROOT / "mercat2_amd" / "csrc" / "mk_lookup.hip").read_text() + (ROOT / "mercat2_amd" / "csrc" / "mk_tsvpieces.h").read_text()
    assert not re.search(r"\b(getenv|mk_env_\w+)\s*\(", text)
