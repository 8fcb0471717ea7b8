"""Two tables combined by key, the parts that need no GPU: header, binding and struct layout of mk_table_op, the op
names, the argument errors of -against / -op, and the rule itself (setop_rule, what the GPU tests compare with)."""
import ctypes as C
import re
from pathlib import Path

import pytest

import setop_rule
from setop_rule import M64
from mercat2_amd import cli, native

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).parent / "golden"
HEADER = (ROOT / "include" / "mercat_hip.h").read_text()


def test_struct_layout_matches_the_header():
    body = re.search(r"typedef struct mk_table_op_t \{(.*?)\} mk_table_op_t;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    want = []
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if stmt:
            ctype, rest = stmt.split(" ", 1)
            want += [(f.strip(), ctype) for f in rest.split(",")]
    ctype = {"uint64_t": C.c_uint64, "int32_t": C.c_int32, "double": C.c_double}
    assert [(name, ctype[t]) for name, t in want] == list(native.TableOp._fields_)
    assert [name for name, _ in want] == ["rows_a", "rows_b", "both", "rows_out", "total_out", "packed_out", "text_out", "slots",
                                          "passes", "op", "s_scan", "s_total"]
    assert C.sizeof(native.TableOp) == 8 * 8 + 2 * 4 + 2 * 8
    assert set(native.TableOp().as_dict()) == {name for name, _ in want}


def test_header_binding_and_library_agree():
    assert re.search(r"int mk_table_op\(mk_ctx\* dst, mk_ctx\* a, mk_ctx\* b, int op, uint64_t min_a, uint64_t min_b, "
                     r"mk_table_op_t\* st\);", HEADER)
    assert "mk_table_op" in native.ABI_SYMBOLS
    fn = native.lib().mk_table_op
    assert fn.restype is C.c_int
    assert fn.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(native.TableOp)]
    assert native.lib().mk_version().decode().split()[1] == "6.1"
    assert fn(None, None, None, 0, 1, 1, None) == -1  # (MK_ERR_ARG before any device is touched)
    assert hasattr(native.Counter, "combine")


def test_ops_name_the_six_codes():
    codes = {name: int(re.search(r"#define MK_OP_%s\s+(\d+)" % name.upper(), HEADER).group(1)) for name in setop_rule.OPS}
    assert native.OPS == codes == dict(zip(("min", "max", "sum", "left", "only", "diff"), range(6)))
    assert (native.OP_MIN, native.OP_MAX, native.OP_SUM, native.OP_LEFT, native.OP_ONLY, native.OP_DIFF) == tuple(range(6))
    assert tuple(cli.AGAINST_OPS) == tuple(native.OPS)


def _refused(argv, capsys) -> str:
    with pytest.raises(SystemExit) as e:
        cli.parseargs(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_cli_argument_errors(tmp_path, capsys):
    folder = tmp_path / "in" / "tsv_nucleotide"
    folder.mkdir(parents=True)
    (folder / "s_counts.tsv").write_bytes(b"k-mer\ts_Count\nACGTA\t3\n")
    base = ["-tsv", str(tmp_path / "in"), "-o", str(tmp_path / "out")]
    table = GOLDEN / "tsv" / "ref_RW1_clean_k5_c10.tsv"
    assert "-op needs -against" in _refused(base + ["-k", "5", "-op", "only"], capsys)
    assert "-against needs -op" in _refused(base + ["-k", "5", "-against", str(table)], capsys)
    assert "invalid choice" in _refused(base + ["-k", "5", "-against", str(table), "-op", "xor"], capsys)
    (tmp_path / "k6.tsv").write_bytes(b"ACGTAC\t3\n")
    assert "holds 6-mers" in _refused(base + ["-k", "5", "-against", str(tmp_path / "k6.tsv"), "-op", "only"], capsys)
    (tmp_path / "raw.tsv").write_bytes(b"AC-TA\t3\nacgta\t1\n")
    assert "neither nucleotide" in _refused(base + ["-k", "5", "-against", str(tmp_path / "raw.tsv"), "-op", "only"], capsys)
    assert "is not valid" in _refused(base + ["-k", "5", "-against", str(tmp_path / "none.tsv"), "-op", "only"], capsys)
    assert "-against_min" in _refused(base + ["-k", "5", "-against", str(table), "-op", "only", "-against_min", "0"], capsys)
    args, _ = cli.parseargs(base + ["-k", "5", "-against", str(table), "-op", "diff", "-against_min", "12"])
    assert (args.against_kind, args.op, args.against_min) == ("nucleotide", "diff", 12)
    args, _ = cli.parseargs(base + ["-k", "5", "-against", str(GOLDEN / "tsv" / "ref_DJ_pro_k5_c10_s1.tsv"), "-op", "min"])
    assert args.against_kind == "protein"


def test_the_rule_on_hand_written_tables():
    a, b = {"x": 5, "y": 2, "z": 9}, {"x": 3, "y": 2, "w": 4}
    assert setop_rule.combine(a, b, "min") == {"x": 3, "y": 2}
    assert setop_rule.combine(a, b, "max") == {"x": 5, "y": 2, "z": 9, "w": 4}
    assert setop_rule.combine(a, b, "sum") == {"x": 8, "y": 4, "z": 9, "w": 4}
    assert setop_rule.combine(a, b, "left") == {"x": 5, "y": 2}
    assert setop_rule.combine(a, b, "only") == {"z": 9}
    assert setop_rule.combine(a, b, "diff") == {"x": 2, "z": 9}
    assert setop_rule.combine(b, a, "diff") == {"w": 4}
    # a count below its threshold is first taken as 0
    assert setop_rule.combine(a, b, "left", 1, 3) == {"x": 5}
    assert setop_rule.combine(a, b, "only", 1, 3) == {"y": 2, "z": 9}
    assert setop_rule.combine(a, b, "max", 6, 1) == {"x": 3, "y": 2, "z": 9, "w": 4}
    assert setop_rule.combine(a, b, "sum", 10, 10) == {}
    # modulo 2^64: a sum that wraps to 0 is no row
    assert setop_rule.combine({"x": M64}, {"x": 1}, "sum") == {}
    assert setop_rule.combine({"x": M64}, {"x": 2}, "sum") == {"x": 1}
    assert setop_rule.combine({"x": M64}, {"x": 1}, "max") == {"x": M64}
    assert setop_rule.combine({"x": 7}, {"x": 7}, "diff") == {}
    assert setop_rule.combine({}, {}, "max") == {} and setop_rule.combine({}, b, "min") == {}
    assert setop_rule.combine({}, b, "sum") == b and setop_rule.combine(a, {}, "only") == a
    assert setop_rule.figures(a, b, "sum") == {"rows_a": 3, "rows_b": 3, "both": 2, "rows_out": 4, "total_out": 25, "passes": 2}
    assert setop_rule.figures(a, b, "left", 1, 3) == {"rows_a": 3, "rows_b": 2, "both": 1, "rows_out": 1, "total_out": 5, "passes": 1}
