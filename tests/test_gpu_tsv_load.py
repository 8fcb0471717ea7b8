"""Count tables read back into GPU tables (mk_load_tsv / mk_load_tsv_text, Counter.load_tsv) and the runs that start from
them (-tsv): files the reference wrote round-trip byte for byte, every table shape loads what it wrote, loads add up,
malformed text is refused with its line and without touching the table, and everything computed from loaded tables
equals what the counted tables give."""
import filecmp
import gzip
import os
import random
from pathlib import Path

import numpy as np
import pytest

from mercat2_amd import cli, native
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden"
NT, AA, RAW = native.ALPHABET_NT2, native.ALPHABET_AA5, native.ALPHABET_RAW
RANGE, NON_ASCII, STATE = -7, -5, -4


def _read(name: str) -> bytes:
    p = GOLDEN / "inputs" / name
    return gzip.open(p, "rb").read() if name.endswith(".gz") else p.read_bytes()


def _tsv(table: dict, name="s", header=True, order=None) -> bytes:
    keys = sorted(table) if order is None else order
    head = "k-mer\t%s_Count\n" % name if header else ""
    return (head + "".join("%s\t%d\n" % (k, table[k]) for k in keys)).encode()


def _golden_alphabet(name: str) -> int:
    return AA if ("_pro_" in name or "_fgs_" in name or name.startswith("edge_protein")) else NT


# ------------------------------------------------------------------------------- files the reference made
@pytest.mark.parametrize("path", sorted((GOLDEN / "tsv").glob("*.tsv")), ids=lambda p: p.name)
def test_committed_tables_round_trip_byte_for_byte(path, tmp_path):
    """Dense bins, one-word keys, AA5, and the rows kept as text (Scaffolds_with-NNN: N and lower case; edge_ws: blanks,
    control bytes and tabs inside keys)."""
    shape = native.tsv_shape(path)
    with native.Counter(shape["k"], _golden_alphabet(path.name)) as ctx:
        info = ctx.load_tsv(path)
        text = path.read_bytes()
        assert info["header"] == 1 and info["column"].endswith("_Count")
        assert info["bytes"] == len(text) and info["lines"] == text.count(b"\n") and info["rows"] == info["lines"] - 1
        assert info["packed_rows"] + info["text_rows"] + info["zero_rows"] == info["rows"] and info["zero_rows"] == 0
        assert info["new_rows"] == info["rows"] == ctx.rows()
        out = tmp_path / "again.tsv"
        assert ctx.write_tsv(out, info["column"][: -len("_Count")]) == info["rows"]
        assert out.read_bytes() == text


# --------------------------------------------------------------------------------- shapes with no committed file
def _synth():
    return native.synth_reads(30_000, 3, 1_500, 150, 4).tobytes()


SHAPES = {
    "nt_k63_two_word": (lambda: _synth(), 63, NT, False, 1),
    "nt_k70_by_reference": (lambda: _synth(), 70, NT, False, 1),
    "raw_k7": (lambda: _read("edge_ws.fa") + _read("A.fasta"), 7, RAW, False, 1),
    "nt_k31_canonical": (lambda: _synth(), 31, NT, True, 1),
    "protein_k8": (lambda: _read("RW1_pro.faa.gz"), 8, AA, False, 1),
    "protein_k13_two_word": (lambda: _read("RW1_pro.faa.gz"), 13, AA, False, 1),
    "nt_k5_dense_with_text_rows": (lambda: _read("Scaffolds_with-NNN.fna.gz"), 5, NT, False, 3),
}


@pytest.mark.parametrize("case", sorted(SHAPES))
def test_every_table_shape_loads_what_it_wrote(case, tmp_path):
    make, k, alphabet, canonical, c = SHAPES[case]
    tsv = tmp_path / "s_counts.tsv"
    with native.Counter(k, alphabet, canonical=canonical) as counted, native.Counter(k, alphabet, canonical=canonical) as loaded:
        counted.count_chunk(make(), c)
        want = counted.to_dict()
        assert len(want) > 100
        counted.write_tsv(tsv, "s")
        info = loaded.load_tsv(tsv)
        assert loaded.stats()["mode_name"] == counted.stats()["mode_name"]
        assert loaded.to_dict() == want
        assert info["rows"] == info["new_rows"] == len(want) and info["column"] == "s_Count" and info["pieces"] == 1
        if loaded.stats()["mode_name"] == "byref":
            assert info["text_rows"] == info["rows"]
        # the same through the text in memory, into a context that guesses nothing: tsv_shape's hint
        other, info2 = native.counter_from_tsv(tsv)
        with other:
            assert other.k == k and other.to_dict() == want
        with native.Counter(k, alphabet, canonical=canonical) as from_bytes:
            assert from_bytes.load_tsv(tsv.read_bytes())["rows"] == len(want)
            assert from_bytes.to_dict() == want


# ------------------------------------------------------------------------------------------------ edge cases
def test_the_key_beside_the_table_round_trips(tmp_path):
    """32 x 'T' is the one-word table's free-slot mark: its count lives beside the table (run_side)."""
    text = b">a\n" + b"T" * 40 + b"ACGTTGCA" * 6 + b"\n>b\n" + b"T" * 33 + b"\n"
    want = cpu_ref.count_text(text, 32, 1)
    assert want["T" * 32] == 11
    tsv = tmp_path / "t_counts.tsv"
    with native.Counter(32, NT) as counted, native.Counter(32, NT) as loaded:
        counted.count_chunk(text, 1)
        counted.write_tsv(tsv, "t")
        info = loaded.load_tsv(tsv)
        assert loaded.to_dict() == want == counted.to_dict() and info["new_rows"] == len(want)
        assert loaded.alpha_stats()["total"] == sum(want.values())
        info = loaded.load_tsv(tsv)  # the side key adds up like every other, and is no new row the second time
        assert info["new_rows"] == 0 and loaded.to_dict() == {k: 2 * v for k, v in want.items()}


@pytest.mark.parametrize("k,alphabet", [(5, NT), (31, NT), (40, NT), (9, RAW)])
def test_large_counts_shuffled_rows_no_header_no_last_newline(k, alphabet, tmp_path):
    rng = random.Random(k)
    keys = sorted({"".join(rng.choice("ACGT") for _ in range(k)) for _ in range(400)})
    table = {key: rng.randrange(1, 1000) for key in keys}
    table[keys[0]] = (1 << 64) - 1
    table[keys[1]] = 1 << 32
    table[keys[2]] = (1 << 63) + 12345
    order = list(keys)
    rng.shuffle(order)
    for header in (True, False):
        for last_newline in (True, False):
            text = _tsv(table, header=header, order=order)
            if not last_newline:
                text = text[:-1]
            with native.Counter(k, alphabet) as ctx:
                info = ctx.load_tsv(text)
                assert info["header"] == int(header) and info["column"] == ("s_Count" if header else "")
                assert info["rows"] == len(table) and info["lines"] == len(table) + int(header) and info["bytes"] == len(text)
                assert ctx.to_dict() == table
                out = tmp_path / ("w_%d_%d.tsv" % (header, last_newline))
                ctx.write_tsv(out, "s")
                assert out.read_bytes() == _tsv(table)


def test_leading_zeros_and_twenty_digits():
    with native.Counter(4, NT) as ctx:
        ctx.load_tsv(b"ACGT\t00000000000000000007\nTTTT\t18446744073709551615\nAAAA\t0018\n")
        assert ctx.to_dict() == {"ACGT": 7, "TTTT": (1 << 64) - 1, "AAAA": 18}


# ------------------------------------------------------------------------------------------------------ sums
def test_loading_a_table_twice_doubles_every_count(tmp_path):
    path = GOLDEN / "tsv" / "A_k31_c1.tsv"
    with native.Counter(31, NT) as ctx:
        first = ctx.load_tsv(path)
        once = ctx.to_dict()
        second = ctx.load_tsv(path)
        assert first["new_rows"] == len(once) and second["new_rows"] == 0 and second["rows"] == first["rows"]
        assert ctx.to_dict() == {k: 2 * v for k, v in once.items()}


@pytest.mark.parametrize("k,alphabet", [(31, NT), (4, NT), (40, NT), (6, RAW)])
def test_two_tables_into_one_context_are_the_keywise_sum(k, alphabet):
    a, b = cpu_ref.count_text(_read("A.fasta"), k, 1), cpu_ref.count_text(_read("B.fasta"), k, 1)
    want = dict(a)
    for key, n in b.items():
        want[key] = want.get(key, 0) + n
    with native.Counter(k, alphabet) as ctx:
        ia = ctx.load_tsv(_tsv(a, "A"))
        ib = ctx.load_tsv(_tsv(b, "B"))
        assert ctx.to_dict() == want
        assert ia["new_rows"] == len(a) and ib["new_rows"] == len(want) - len(a)


@pytest.mark.parametrize("k,alphabet", [(6, NT), (31, NT), (40, NT), (6, RAW)])
def test_a_key_listed_twice_adds_up_and_zero_rows_are_skipped(k, alphabet):
    rng = random.Random(7 * k)
    keys = ["".join(rng.choice("ACGTN") for _ in range(k)) for _ in range(300)]
    rows = [(rng.choice(keys), rng.choice([0, 0, 1, 5, 1 << 40])) for _ in range(3000)]
    want = {}
    for key, n in rows:
        if n:
            want[key] = want.get(key, 0) + n
    text = "".join("%s\t%d\n" % r for r in rows).encode()
    with native.Counter(k, alphabet) as ctx:
        info = ctx.load_tsv(text)
        assert info["header"] == 0 and info["rows"] == len(rows)
        assert info["zero_rows"] == sum(1 for _, n in rows if not n)
        assert info["new_rows"] == len(want)
        assert ctx.to_dict() == want
    with native.Counter(4, NT) as ctx:  # a table of zero rows only stays empty, and writes no file
        info = ctx.load_tsv(b"k-mer\tz_Count\nACGT\t0\nAAAN\t0\n")
        assert (info["rows"], info["zero_rows"], info["new_rows"], ctx.rows()) == (2, 2, 0, 0)


# ---------------------------------------------------------------------------------------------------- pieces
def test_a_table_loaded_in_pieces_equals_the_one_piece_load(tmp_path):
    data = native.synth_reads(120_000, 11, 12_000, 150, 12).tobytes()
    tsv = tmp_path / "big_counts.tsv"
    with native.Counter(31, NT) as counted:
        counted.count_chunk(data, 1)
        rows = counted.write_tsv(tsv, "big")
        want = counted.export()
    assert rows >= 200_000
    with native.Counter(31, NT) as whole, native.Counter(31, NT) as pieces, native.Counter(31, RAW) as text_pieces:
        one = whole.load_tsv(tsv)
        many = pieces.load_tsv(tsv, piece_bytes=64 << 10)
        assert one["pieces"] == 1 and many["pieces"] > 1
        assert many["pieces"] >= os.path.getsize(tsv) // (64 << 10)
        for f in ("bytes", "lines", "rows", "packed_rows", "text_rows", "zero_rows", "new_rows", "header"):
            assert one[f] == many[f], f
        for ctx in (whole, pieces):
            got = ctx.export()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        out = tmp_path / "again.tsv"
        pieces.write_tsv(out, "big")
        assert filecmp.cmp(out, tsv, shallow=False)
        # the by-reference import, piece after piece, from the text in memory
        t = text_pieces.load_tsv(tsv.read_bytes(), piece_bytes=64 << 10)
        assert t["pieces"] > 1 and t["text_rows"] == t["rows"] == rows
        got = text_pieces.export()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# -------------------------------------------------------------------------------------------------- refusals
GOOD = ["ACGTA\t5", "CCGTA\t7", "GGGTA\t1", "TTGTA\t2", "TTTTT\t9", "ANGTA\t3"]
BAD_LINES = {
    "key_too_short": (b"ACGT\t5", RANGE),
    "key_too_long": (b"ACGTAC\t5", RANGE),
    "missing_tab": (b"ACGTA5", RANGE),
    "empty_count": (b"ACGTA\t", RANGE),
    "non_digit": (b"ACGTA\t5x", RANGE),
    "minus_sign": (b"ACGTA\t-5", RANGE),
    "twenty_one_digits": (b"ACGTA\t" + b"1" * 21, RANGE),
    "above_u64": (b"ACGTA\t18446744073709551616", RANGE),
    "carriage_return": (b"ACGTA\t5\r", RANGE),
    "empty_line": (b"", RANGE),
    "high_byte_in_key": (b"AC\xc3\xa9A\t5", NON_ASCII),
    "high_byte_in_count": (b"ACGTA\t5\xff", NON_ASCII),
}


def _with_bad_line(bad: bytes, at: int, rows: int, header: bool):
    """(text, 1-based line number of the bad line): ``rows`` good rows, the bad one put in front of good row ``at``."""
    lines = [GOOD[i % len(GOOD)].encode() for i in range(rows)]
    lines.insert(at, bad)
    head = [b"k-mer\ts_Count"] if header else []
    return b"\n".join(head + lines) + b"\n", at + 1 + len(head)


@pytest.mark.parametrize("alphabet", [NT, RAW], ids=["dense", "byref"])
@pytest.mark.parametrize("case", sorted(BAD_LINES))
def test_a_malformed_table_is_refused_and_leaves_the_context_as_it_was(case, alphabet):
    bad, code = BAD_LINES[case]
    before = {"AAAAA": 4, "ACGTA": 1, "NNNNN": 2}
    with native.Counter(5, alphabet) as ctx:
        ctx.load_tsv(_tsv(before))
        rows0, (k0, c0) = ctx.rows(), ctx.export()
        for header, at in ((True, 3), (False, 5), (True, 40)):
            text, line = _with_bad_line(bad, at, 40, header)
            with pytest.raises(native.MercatHipError) as e:
                ctx.load_tsv(text)
            assert e.value.code == code, str(e.value)
            assert ("line %d:" % line) in str(e.value), str(e.value)
            if code == NON_ASCII:
                assert isinstance(e.value, native.NonAsciiInput)
            k1, c1 = ctx.export()  # nothing of the refused text is in the table, and the context goes on working
            assert ctx.rows() == rows0 and np.array_equal(k0, k1) and np.array_equal(c0, c1)
        ctx.load_tsv(b"AAAAA\t1\n")
        assert ctx.to_dict() == dict(before, AAAAA=5)


@pytest.mark.parametrize("k,alphabet", [(5, NT), (31, NT), (40, NT), (5, RAW)])
@pytest.mark.parametrize("case", ["key_too_short", "non_digit", "above_u64", "carriage_return", "high_byte_in_key"])
def test_a_refusal_in_a_late_piece_spoils_the_context_until_reset(case, k, alphabet):
    bad, code = BAD_LINES[case]
    bad = bad.replace(b"ACGTA", b"ACGTA" + b"C" * (k - 5)).replace(b"ACGT\t", b"ACGT" + b"C" * (k - 5) + b"\t")
    bad = bad.replace(b"AC\xc3\xa9A", b"AC\xc3\xa9A" + b"C" * (k - 5))
    rng = random.Random(3)
    keys = ["".join(rng.choice("ACGT") for _ in range(k)) for _ in range(6000)]
    lines = [("%s\t%d" % (key, 1 + i % 9)).encode() for i, key in enumerate(keys)]
    at = 5500
    lines.insert(at, bad)
    text = b"k-mer\ts_Count\n" + b"\n".join(lines) + b"\n"
    with native.Counter(k, alphabet) as ctx:
        with pytest.raises(native.MercatHipError) as e:
            ctx.load_tsv(text, piece_bytes=8192)
        assert e.value.code == code and ("line %d:" % (at + 2)) in str(e.value), str(e.value)
        for call in (ctx.rows, ctx.export, lambda: ctx.load_tsv(b""), lambda: ctx.count_chunk(b">a\nACGTACGT\n", 1)):
            with pytest.raises(native.MercatHipError) as e2:  # never silently partial
                call()
            assert e2.value.code == STATE
        ctx.reset()
        assert ctx.rows() == 0
        want = {}
        for i, key in enumerate(keys):
            want[key] = want.get(key, 0) + 1 + i % 9
        info = ctx.load_tsv(b"\n".join(l for l in lines if l is not bad) + b"\n", piece_bytes=8192)
        assert info["pieces"] > 1 and ctx.to_dict() == want


def test_a_refusal_in_the_first_of_several_pieces_changes_nothing():
    lines = [GOOD[i % len(GOOD)].encode() for i in range(5000)]
    lines[10] = b"ACGTA\tx"
    with native.Counter(5, NT) as ctx:
        ctx.load_tsv(b"ACGTA\t3\n")
        with pytest.raises(native.MercatHipError) as e:
            ctx.load_tsv(b"\n".join(lines) + b"\n", piece_bytes=4096)
        assert e.value.code == RANGE and "line 11:" in str(e.value)
        assert ctx.to_dict() == {"ACGTA": 3}


def test_a_line_longer_than_a_piece_is_refused():
    with native.Counter(5, NT) as ctx:
        with pytest.raises(native.MercatHipError) as e:
            ctx.load_tsv(b"ACGTA\t1\nCCCCC\t2\n" + b"A" * 5000 + b"\t1\nGGGGG\t1\n", piece_bytes=1024)
        assert e.value.code == RANGE and "line 3:" in str(e.value)
        assert ctx.rows() == 0
        ctx.load_tsv(b"ACGTA\t1\n")
        assert ctx.to_dict() == {"ACGTA": 1}


def test_wrong_k_for_the_context_names_the_first_data_row():
    """Line 1 is a header when it is no data row OF THIS k: a 31-mer table offered to a 21-mer context is refused at line 2."""
    with native.Counter(21, NT) as ctx:
        with pytest.raises(native.MercatHipError) as e:
            ctx.load_tsv(GOLDEN / "tsv" / "A_k31_c1.tsv")
        assert e.value.code == RANGE and "line 2:" in str(e.value) and ctx.rows() == 0
    with native.Counter(5, NT) as ctx:
        with pytest.raises(native.MercatHipError) as e:
            ctx.load_tsv(GOLDEN / "tsv" / "no_such_file.tsv")
        assert e.value.code == -6


# --------------------------------------------------------------------------------------- downstream equality
DOWNSTREAM = {
    "nucleotide_k31": (31, NT, 1, ["A.fasta", "B.fasta", "C.fasta", "edge_reads.fna"]),
    "protein_k5": (5, AA, 10, ["DJ_pro.faa.gz", "RW1_pro.faa.gz", "RW2_pro.faa.gz", "GIC31_pro.faa.gz"]),
}


@pytest.mark.parametrize("case", sorted(DOWNSTREAM))
def test_everything_computed_from_loaded_tables_equals_the_counted_tables(case, tmp_path):
    k, alphabet, c, files = DOWNSTREAM[case]
    counted, loaded = [], []
    try:
        for i, name in enumerate(files):
            ctx = native.Counter(k, alphabet)
            counted.append(ctx)
            ctx.count_chunk(_read(name), c)
            tsv = tmp_path / ("s%d_counts.tsv" % i)
            assert ctx.write_tsv(tsv, "s%d" % i) > 0
            other = native.Counter(k, alphabet)
            loaded.append(other)
            other.load_tsv(tsv)
        km_a, mx_a = native.merged_export(counted)
        km_b, mx_b = native.merged_export(loaded)
        assert np.array_equal(km_a, km_b) and np.array_equal(mx_a, mx_b)
        assert native.gram(counted) == native.gram(loaded)
        pa, pb = native.pair_stats(counted), native.pair_stats(loaded)
        for f in ("dot", "l1", "sums", "rows", "constant_row"):
            assert pa[f] == pb[f], f
        for f in ("cheb", "neq", "both"):
            assert np.array_equal(pa[f], pb[f]), f
        for x, y in zip(counted, loaded):
            sa, sb = x.alpha_stats(), y.alpha_stats()
            # integers, and a sum of squares far below 2^53: exact whatever the order of the additions
            for f in ("observed", "total", "freq", "sum_sq"):
                assert sa[f] == sb[f], f
            # sum of count * ln(count) in f64, added in the order of the slots, and two tables lay the same rows out
            # differently: n additions are off by at most n * 2^-53 relative (n < 2^20 rows here: 2^-33 ~ 1.2e-10)
            assert sb["sum_clnc"] == pytest.approx(sa["sum_clnc"], rel=2e-10, abs=0)
    finally:
        for ctx in counted + loaded:
            ctx.close()


# ------------------------------------------------------------------------------------------------------ CLI
PROTEOMES = ["DJ_pro.faa.gz", "GIC31_pro.faa.gz", "RW1_pro.faa.gz", "RW2_pro.faa.gz", "Rleg_pro.faa.gz"]


def _files_under(root: Path) -> list:
    return sorted(str(p.relative_to(root)) for p in root.rglob("*") if p.is_file())


def _assert_same_folders(a: Path, b: Path):
    assert _files_under(a) == _files_under(b)
    for rel in _files_under(a):
        assert (a / rel).read_bytes() == (b / rel).read_bytes(), rel


def _count(files, out: Path, *more):
    assert cli.main(["-i"] + [str(GOLDEN / "inputs" / f) for f in files] + ["-k", "5", "-c", "10", "-pca", "-o", str(out)] + list(more)) == 0


def test_cli_reports_from_a_result_folder_without_recounting(tmp_path, capsys):
    out1, out2, out3 = tmp_path / "out1", tmp_path / "out2", tmp_path / "out3"
    _count(PROTEOMES, out1)
    capsys.readouterr()
    assert cli.main(["-tsv", str(out1), "-k", "5", "-pca", "-o", str(out2)]) == 0
    printed = capsys.readouterr().out
    assert printed.count("Loaded ") == 5 and "Significant k-mers" not in printed and "already filtered" in printed
    files = _files_under(out1)
    assert "combined_protein.tsv" in files and "combined_protein_T.tsv" in files and os.path.join("pca_protein", "pca.tsv") in files
    assert sum(f.startswith("tsv_protein" + os.sep) for f in files) == 5 and any(f.startswith("report" + os.sep) for f in files)
    _assert_same_folders(out1, out2)
    # the new folder is a complete result folder: it loads in turn, and so does its tsv_protein folder by itself
    assert cli.main(["-tsv", str(out2 / "tsv_protein"), "-k", "5", "-pca", "-o", str(out3)]) == 0
    _assert_same_folders(out1, out3)


def test_cli_extends_a_cohort_by_one_sample(tmp_path):
    out5, out4, ext = tmp_path / "out5", tmp_path / "out4", tmp_path / "ext"
    _count(PROTEOMES, out5)
    _count(PROTEOMES[:4], out4)
    _count(PROTEOMES[4:], ext, "-tsv", str(out4))
    _assert_same_folders(out5, ext)
    with pytest.raises(SystemExit) as e:  # -k must be the tables' k
        cli.main(["-tsv", str(out4), "-k", "6", "-o", str(tmp_path / "never")])
    assert e.value.code == 2 and not (tmp_path / "never").exists()
    with pytest.raises(SystemExit) as e:  # one sample, given twice
        _count(PROTEOMES[:1], tmp_path / "never", "-tsv", str(out4))
    assert e.value.code == 2
