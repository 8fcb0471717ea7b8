"""Reads screened against the GPU tables (mk_screen_text / mk_screen_device, Counter.screen*, kmers.screen_reads,
report.write_screen_tsv, -screen).  Expected rows never come from the code under test: the table is a dict made by the CPU
oracle (or a committed reference table), the records of the screened text come from the reference's own line loop
written out below, and a row is plain Python over ``dict.get(window, 0)``.  Equality is exact in all five columns."""
import ctypes
import functools
import io
import random
import shutil
from pathlib import Path

import numpy as np
import pytest

import walk_seams
from conftest import read_input
from mercat2_amd import cli, kmers, native, report
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden"
NT, AA, RAW = native.ALPHABET_NT2, native.ALPHABET_AA5, native.ALPHABET_RAW
ARG, STATE, NON_ASCII, RANGE = -1, -4, -5, -7
COMP = str.maketrans("ACGT", "TGCA")


def ref_records(text: bytes):
    """[(name, sequence)] by the reference's line loop (lib/mercat2_kmers.py:49-69): text mode, strip(), startswith('>'),
    replace('*', '').  Records with an empty sequence are kept; sequence in front of the first header is a record named
    ''."""
    recs = []
    for line in io.TextIOWrapper(io.BytesIO(text), encoding="latin-1", newline=None):
        line = line.strip()
        if line.startswith(">"):
            words = line[1:].split()
            recs.append([words[0] if words else "", ""])
        else:
            piece = line.replace("*", "")
            if not recs and piece:
                recs.append(["", ""])
            if recs:
                recs[-1][1] += piece
    return [(name, seq) for name, seq in recs]


def expected_rows(text: bytes, table: dict, k: int, at_least: int = 1, fold: bool = False):
    rows = []
    for _, seq in ref_records(text):
        counts = []
        for i in range(len(seq) - k + 1):
            w = seq[i:i + k]
            if fold and set(w) <= set("ACGT"):
                w = min(w, w.translate(COMP)[::-1])
            counts.append(table.get(w, 0))
        rows.append([len(counts), sum(1 for c in counts if c >= at_least), sum(counts) % (1 << 64),
                     min(counts, default=0), max(counts, default=0)])
    return rows


def check(ctx, text: bytes, table: dict, at_least: int = 1, fold=None, folded_table: bool = False, **kw):
    info = {}
    got = ctx.screen(text, at_least, fold=fold, info=info, **kw)
    want = expected_rows(text, table, ctx.k, at_least, folded_table)
    assert got.shape == (len(want), 5) and got.dtype == np.uint64
    assert got.tolist() == want
    assert info["records"] == len(want) and info["bytes"] == len(text)
    assert info["windows"] == sum(r[0] for r in want) and info["hits"] == sum(r[1] for r in want)
    assert info["packed_windows"] + info["text_windows"] == info["windows"]
    return got, info


def dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def wrap(seq, width):
    return "".join(seq[i:i + width] + "\n" for i in range(0, len(seq), width))


# --------------------------------------------------------------------------------------------- record shapes
@functools.lru_cache(maxsize=None)
def shapes_text(k: int, headless: bool) -> bytes:
    """Every record shape of the issue in one text; ends in a header."""
    rng = random.Random(1000 * k)
    long_seq = dna(rng, 40_011)
    t = [dna(random.Random(k + 1), k + 2) + "\n" if headless else "  \n\t\n \x0b\n"]
    t += [">km1 a b\n" + dna(rng, k - 1) + "\n", ">k\n" + dna(rng, k) + "\n", "  >kp1\tx\n" + dna(rng, k + 1) + "\n"]
    t += [">h1\n>h2\n" + dna(rng, k + 3) + "\n", ">\n" + dna(rng, k + 1) + "\n"]
    t += [">wrapped\n" + wrap(dna(rng, 3 * k + 5), 7)]
    s = dna(rng, 2 * k + 4)
    t += [">crlf\r\n" + s[:5] + "\r\n" + s[5:] + "\r\n", ">cr\r" + dna(rng, k + 2) + "\r" + dna(rng, 3) + "\r"]
    s = dna(rng, k + 6)
    t += [">star\n" + s[:3] + "*" + s[3:] + "**\n*\n", ">blank\n  " + dna(rng, 5) + " \t" + dna(rng, k + 1) + "  \n"]
    t += [">s%d\n%s\n" % (i, dna(rng, k + i % 4)) for i in range(300)]  # many records in one lane's run, in one wave
    t += [">long\n" + wrap(long_seq, 60)]                                # lanes, waves, workgroups: the halo, the wave flush
    t += [">t%d\n%s\n" % (i, dna(rng, k + 1 + i)) for i in range(3)]
    t += [">copy of a piece of long\n" + long_seq[17_000:17_000 + 2 * k] + "\n", ">last one"]
    return "".join(t).encode()


@functools.lru_cache(maxsize=None)
def other_text(k: int) -> bytes:
    """Another text that shares half of the long record: a table of it gives hits and misses."""
    rng = random.Random(77 + k)
    long_seq = [r for r in ref_records(shapes_text(k, False)) if r[0] == "long"][0][1]
    return (">x\n" + wrap(dna(rng, 5_000), 70) + ">y\n" + wrap(long_seq[:20_000], 80)).encode()


@functools.lru_cache(maxsize=None)
def table_of(text: bytes, k: int, c: int = 1) -> dict:
    return cpu_ref.count_text(text, k, c)


@pytest.mark.parametrize("own", [True, False], ids=["own_table", "other_table"])
@pytest.mark.parametrize("headless", [False, True], ids=["blanks_first", "headless"])
@pytest.mark.parametrize("k", [5, 31])
def test_record_shapes(k, headless, own):
    text = shapes_text(k, headless)
    source = text if own else other_text(k)
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(source, 1)
        got, info = check(ctx, text, table_of(source, k))
        assert info["headless"] == (1 if headless else 0) and info["pieces"] == 1
        names = [name for name, _ in ref_records(text)]
        assert kmers.record_names(text) == names and names[-1] == "last" and got[-1].tolist() == [0] * 5
        at = names.index("km1")
        assert [int(r[0]) for r in got[at:at + 5]] == [0, 1, 2, 0, 4]  # k - 1, k, k + 1; a header behind a header
        assert int(got[names.index("long")][0]) == 40_011 - k + 1
        if own:
            assert (got[:, 1] == got[:, 0]).all() and (got[got[:, 0] > 0, 3] >= 1).all()
        else:
            assert 0 < int(got[:, 1].sum()) < int(got[:, 0].sum())
        if k == 31:  # the blank kept inside a sequence line: windows over it are text keys
            assert info["text_windows"] > 0 and info["packed_windows"] > 0


def test_pieces():
    k = 31
    text = shapes_text(k, True)
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(other_text(k), 1)
        whole, info = check(ctx, text, table_of(other_text(k), k))
        # (the long record is two thirds of the text and is never split: its piece is as long as it is)
        five, info5 = check(ctx, text, table_of(other_text(k), k), piece_bytes=len(text) // 12)
        small, info_s = check(ctx, text, table_of(other_text(k), k), piece_bytes=1024)  # far below the long record
        assert info["pieces"] == 1 and 4 <= info5["pieces"] <= 6 and info_s["pieces"] > 8
        assert whole.tolist() == five.tolist() == small.tolist()
        assert info5["headless"] == info_s["headless"] == 1


# --------------------------------------------------------------------------------------- the walk's own seams
@functools.lru_cache(maxsize=None)
def seam_rows(k: int, at_least: int = 1):
    return expected_rows(walk_seams.seam_text(k), table_of(walk_seams.other_text(k), k), k, at_least)


@pytest.mark.parametrize("k,at_least", [(5, 17), (31, 1)])  # (nearly every 5-mer is in any table: hits and misses by its counts)
def test_walk_seams(k, at_least):
    """Record boundaries on every lane, wave and tile seam of the walk (tests/walk_seams.py), in one piece and in many."""
    text, source, want = walk_seams.seam_text(k), walk_seams.other_text(k), seam_rows(k, at_least)
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(source, 1)
        for piece_bytes in (0, len(text) // 12):
            info = {}
            got = ctx.screen(text, at_least, info=info, piece_bytes=piece_bytes)
            assert got.dtype == np.uint64 and got.tolist() == want
            assert info["records"] == len(want) and (info["pieces"] > 8 if piece_bytes else info["pieces"] == 1)
            assert info["windows"] == sum(r[0] for r in want) and info["hits"] == sum(r[1] for r in want)
            assert 0 < info["hits"] < info["windows"] and info["packed_windows"] == info["windows"]
        names = [name for name, _ in ref_records(text)]
        assert int(got[names.index("long")][0]) > 3 * walk_seams.TILE - k


@pytest.mark.parametrize("k,at_least,min_ppm", [(5, 17, 500_000), (31, 1, 400_000)])
def test_walk_seams_filter(k, at_least, min_ppm):
    """The same text through Counter.filter and back: the rows, the decision and the bytes of the records it keeps."""
    text, source, want = walk_seams.seam_text(k), walk_seams.other_text(k), seam_rows(k, at_least)
    want_keep = [w > 0 and h >= 1 and h * 1_000_000 >= min_ppm * w for w, h, _, _, _ in want]
    recs = [b">" + r for r in text.split(b">")[1:]]
    assert len(recs) == len(want) and 0 < sum(want_keep) < len(want_keep)
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(source, 1)
        for piece_bytes in (0, len(text) // 12):
            info = {}
            kept, keep, rows = ctx.filter(text, at_least, 1, min_ppm, piece_bytes=piece_bytes, info=info)
            assert rows.tolist() == want and keep.tolist() == want_keep
            assert kept == b"".join(r for r, k_ in zip(recs, want_keep) if k_)
            assert info["pieces"] > 8 if piece_bytes else info["pieces"] == 1
        dropped, _, _ = ctx.filter(text, at_least, 1, min_ppm, invert=True)
        assert dropped == b"".join(r for r, k_ in zip(recs, want_keep) if not k_)


# ----------------------------------------------------------------------------------------------- table shapes
def nt_text(seed: int) -> bytes:
    reads = native.synth_reads(6_000, seed, 120, 150, seed + 1).tobytes()
    return reads + (b">side\nACG" + b"T" * 75 + b"GCA\n>odd\n" + b"ACGTTGCANGGATCCATGNAacgtACGGT*CAGT" * 12 +
                    b"\n>lower\nacgtacgtacgtnnnnACGTACGTAGCTAGCTAGCATCGATCGATCAGCTACGATCGATCGACTAGCTAGCTAGCATGCATGCCCATAGAGACCAGATTTAGAG\n")


def aa_text(seed: int) -> bytes:
    rng = random.Random(seed)
    letters = "ACDEFGHIKLMNPQRSTVWY"
    recs = [">p%d\n%s\n" % (i, wrap("".join(rng.choice(letters) for _ in range(rng.randrange(20, 400))), 60)) for i in range(40)]
    recs.append(">odd\nMKV-LLAX*BZJUOacdeMKVLLAGGHHWWYYPPQQRRSSTTVVMKVLLAAGGHHWWYY.PPQQRRSSTTVVKKLL\n")
    return "".join(recs).encode() + read_input("edge_protein.faa")[:6_000]


SHAPES = [("nt", NT, k) for k in (5, 11, 31, 32, 33, 63, 64, 70)] + [("aa", AA, k) for k in (5, 12, 13, 25)] + [("raw", RAW, 9)]


@pytest.mark.parametrize("kind,alphabet,k", SHAPES, ids=["%s_k%d" % (s[0], s[2]) for s in SHAPES])
def test_every_table_shape(kind, alphabet, k):
    make = aa_text if kind == "aa" else nt_text
    text = make(3)
    # the table: the first half of the text, the run of T, and a piece of the record that holds bytes outside the alphabets
    source = text[: len(text) // 2] + b"\n>side\nACG" + b"T" * 75 + b"GCA\n>x\n" + \
        (b"MKV-LLAX*BZJUOacdeMKVLLAGGHHWWYYPPQQRR" if kind == "aa" else b"ACGTTGCANGGATCCATGNAacgtACGGT*CAGT" * 3) + b"\n"
    table = table_of(source, k)
    with native.Counter(k, alphabet) as ctx:
        ctx.count_chunk(source, 1)
        got, info = check(ctx, text, table)
        assert 0 < info["hits"] < info["windows"]
        if alphabet == RAW or k == 70:
            assert info["packed_windows"] == 0
        else:  # N, lower-case runs, '-', '.': answered from the by-reference table
            assert info["text_windows"] > 0 and info["packed_windows"] > 0
            odd = [i for i, (name, _) in enumerate(ref_records(text)) if name in ("odd", "lower")]
            assert odd and all(int(got[i][0]) > 0 for i in odd)
        if kind == "nt" and k in (31, 32):  # the run of T: at k = 32 the key kept beside the one-word table
            assert table.get("T" * k, 0) >= 1
        check(ctx, text, table, at_least=2)


# -------------------------------------------------------------------------------------------------------- fold
@pytest.mark.parametrize("k", [31, 63])
def test_fold(k):
    rng = random.Random(k)
    read = dna(rng, 150)
    source = nt_text(5)
    text = nt_text(5)[:9_000] + ("\n>fwd\n%s\n>rev\n%s\n>n\n%sN%s\n" % (read, read.translate(COMP)[::-1], read[:70], read[70:])).encode()
    source += (">r\n%s\n" % read).encode()
    folded = cpu_ref.canonical_fold(table_of(source, k))
    with native.Counter(k, NT, canonical=True) as ctx:
        ctx.count_chunk(source, 1)
        assert ctx.to_dict() == folded
        got, info = check(ctx, text, folded, folded_table=True)  # fold=None: as the context counts
        names = [name for name, _ in ref_records(text)]
        fwd, rev = got[names.index("fwd")].tolist(), got[names.index("rev")].tolist()
        assert fwd == rev and fwd[0] == fwd[1] == 150 - k + 1
        assert info["folded"] > 0
        check(ctx, text, folded, fold=True, folded_table=True)
        check(ctx, text, folded, fold=False)  # taken as they stand: the windows of the other strand miss
    with native.Counter(k, NT) as plain:
        with pytest.raises(native.MercatHipError) as e:
            plain.screen(text, fold=True)
        assert e.value.code == ARG


# ------------------------------------------------------------------------------------------ at_least, contract
def test_at_least():
    k, text = 11, nt_text(3)
    table = table_of(text, k)
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(text, 1)
        for at_least in (1, 2, max(table.values()) + 1):
            got, _ = check(ctx, text, table, at_least=at_least)
        assert not got[:, 1].any() and got[:, 0].any()
        with pytest.raises(native.MercatHipError) as e:
            ctx.screen(text, 0)
        assert e.value.code == ARG


def _raw_screen(ctx, text: bytes, cap: int, at_least: int = 1):
    rows = np.full((cap + 1, 5), 0xABAB, dtype=np.uint64)
    n = ctypes.c_size_t(0)
    rc = native.lib().mk_screen_text(ctx._h, text, len(text), 0, 0, at_least, rows.ctypes.data, cap, ctypes.byref(n), None)
    return rc, n.value, rows


def test_contract():
    k, text = 31, shapes_text(31, False)
    table = table_of(text, k)
    with native.Counter(k, NT) as ctx:
        # an empty table: the windows are there, nothing else
        got = ctx.screen(text)
        want = [[r[0], 0, 0, 0, 0] for r in expected_rows(text, {}, k)]
        assert got.tolist() == want and got[:, 0].any()
        ctx.count_chunk(text, 1)
        before, size = ctx.to_dict(), ctx.rows()
        stats = ctx.stats()
        first, _ = check(ctx, text, table)
        again, _ = check(ctx, text, table)
        assert first.tolist() == again.tolist()
        assert ctx.rows() == size and ctx.to_dict() == before == table
        after = ctx.stats()
        assert all(after[f] == stats[f] for f in ("raw_bytes", "symbols", "windows", "exotic_windows", "chunks", "survivors"))
        # an empty text
        info = {}
        assert ctx.screen(b"", info=info).shape == (0, 5) and info["records"] == 0
        rc, n, _ = _raw_screen(ctx, b"", 0)
        assert (rc, n) == (0, 0)
        # cap short by one row: the needed size, and the row past cap untouched
        records = len(first)
        rc, n, rows = _raw_screen(ctx, text, records - 1)
        assert rc == RANGE and n == records and (rows[records - 1] == 0xABAB).all()
        rc, n, rows = _raw_screen(ctx, text, records)
        assert rc == 0 and n == records and rows[:records].tolist() == first.tolist() and (rows[records] == 0xABAB).all()
        # an open chunk
        assert ctx._L.mk_chunk_begin(ctx._h) == 0
        with pytest.raises(native.MercatHipError) as e:
            ctx.screen(text)
        assert e.value.code == STATE
        assert ctx._L.mk_chunk_end(ctx._h, 1) == 0
        # a byte >= 0x80: refused in a sequence line, fine in a header line
        with pytest.raises(native.NonAsciiInput):
            ctx.screen(b">a\nACGT\xc3\xa9ACGT\n")
        assert ctx.screen(b">a \xc3\xa9\nACGT\n").tolist() == [[0, 0, 0, 0, 0]]
        assert ctx.to_dict() == table


@pytest.mark.parametrize("lead", [0, 3])
def test_screen_device_agrees(lead):
    import torch
    k, text = 31, shapes_text(31, True)
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(other_text(k), 1)
        want = ctx.screen(text, 2)
        d_text = torch.from_numpy(np.frombuffer(b"#" * lead + text, dtype=np.uint8).copy()).cuda()  # (lead: an unaligned address)
        d_rows = torch.full((len(want) + 1, 5), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        info = ctx.screen_device(d_text.data_ptr() + lead, len(text), d_rows.data_ptr(), len(want), 2)
        got = d_rows.cpu().numpy().view(np.uint64)
        assert info["records"] == len(want) and got[:-1].tolist() == want.tolist() and (got[-1] == np.uint64(2**64 - 1)).all()
        assert want.tolist() == expected_rows(text, table_of(other_text(k), k), k, 2)
        with pytest.raises(native.MercatHipError) as e:
            ctx.screen_device(d_text.data_ptr() + lead, len(text), d_rows.data_ptr(), len(want) - 1, 2)
        assert e.value.code == RANGE


# ---------------------------------------------------------------------------------------------- above the ABI
def _tsv_rows(path: Path, k: int) -> dict:
    lines = path.read_bytes().split(b"\n")[1:]
    return {line[:k].decode(): int(line[k + 1:]) for line in lines if line}


def test_screen_reads_fastq_and_fasta():
    table = _tsv_rows(GOLDEN / "tsv" / "ref_Test_R1_k5_c10.tsv", 5)
    with native.Counter(5, NT) as ctx:
        ctx.count_chunk(read_input("Test_R1.fna.gz"), 10)
        assert ctx.to_dict() == table
        names_q, rows_q = kmers.screen_reads(ctx, GOLDEN / "inputs" / "Test_R1.fastq.gz")
        names_a, rows_a = kmers.screen_reads(ctx, GOLDEN / "inputs" / "Test_R1.fna.gz")
        assert names_q == names_a and rows_q.tolist() == rows_a.tolist() and len(names_a) > 10
        fasta = read_input("Test_R1.fna.gz")
        assert names_a == [name for name, _ in ref_records(fasta)]
        assert rows_a.tolist() == expected_rows(fasta, table, 5)


def test_write_screen_tsv(tmp_path):
    text = b">a x\nACGTACGTAC\n>b\nAC\n"
    with native.Counter(5, NT) as ctx:
        ctx.count_chunk(text, 1)
        names, rows = kmers.screen_reads(ctx, _write(tmp_path / "r.fa", text), 2)
    assert names == ["a", "b"] and rows.tolist() == [[6, 4, 10, 1, 2], [0, 0, 0, 0, 0]]
    assert report.write_screen_tsv(tmp_path / "s.tsv", names, rows) == 2
    assert (tmp_path / "s.tsv").read_bytes() == b"record\twindows\thits\tsum\tmin\tmax\na\t6\t4\t10\t1\t2\nb\t0\t0\t0\t0\t0\n"


def _write(path: Path, data: bytes) -> Path:
    path.write_bytes(data)
    return path


def test_cli_screen(tmp_path):
    old = tmp_path / "old" / "tsv_nucleotide"
    old.mkdir(parents=True)
    shutil.copyfile(GOLDEN / "tsv" / "ref_Test_R1_k5_c10.tsv", old / "Test_R1_counts.tsv")
    table = _tsv_rows(GOLDEN / "tsv" / "ref_Test_R1_k5_c10.tsv", 5)
    reads = _write(tmp_path / "reads.fna", b">r1 first\nACGTACGTTTGACCA\nGGATC\n>r2\nACG\n>r3\nNNNNNNNACGTA\n")
    out = tmp_path / "out"
    assert cli.main(["-tsv", str(tmp_path / "old"), "-k", "5", "-screen", str(reads), "-screen_min", "2", "-o", str(out)]) == 0
    want = b"record\twindows\thits\tsum\tmin\tmax\n"
    for (name, _), row in zip(ref_records(reads.read_bytes()), expected_rows(reads.read_bytes(), table, 5, 2)):
        want += name.encode() + b"".join(b"\t%d" % v for v in row) + b"\n"
    assert (out / "screen_nucleotide" / "Test_R1_screen.tsv").read_bytes() == want
    assert not (out / "screen_protein").exists()
    # a missing file ends the run before anything is counted or written
    with pytest.raises(SystemExit):
        cli.main(["-tsv", str(tmp_path / "old"), "-k", "5", "-screen", str(tmp_path / "nope.fa"), "-o", str(tmp_path / "out2")])
    assert not (tmp_path / "out2").exists()
